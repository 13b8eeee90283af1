// VerifyMultipleStream of include/milagro_bls.hpp (mbls_stream_create_vm_committee, mbls_stream_submit_vm): three gossip batches -- aggregates over committees
// mixed with sets under single keys, one batch of single-key sets only, one batch with a wrong participation bit -- share one round and give the bools and the
// per-set answers of CommitteeTable::verify_multiple_aggregate_signatures_locate on each batch alone, with the generator left where that method leaves it on
// the accepted batches; what does not fit is refused. Exit code 0 = all passed.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include "milagro_bls.hpp"
using namespace milagro_bls;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); fails++; } } while (0)

struct ByteRng { std::mt19937 g; explicit ByteRng(uint32_t seed) : g(seed) {} uint8_t operator()() { return uint8_t(g()); } };

int main() {
    std::mt19937 gen(9917);
    auto rand_sk = [&] { Bytes b(32); for (auto& v : b) v = uint8_t(gen()); b[0] &= 0x3f; b[31] |= 1; return SecretKey::from_bytes(b); };
    const int NK = 20;
    std::vector<SecretKey> sks; std::vector<PublicKey> pks; Bytes wire;
    for (int i = 0; i < NK; i++) { sks.push_back(rand_sk()); pks.push_back(PublicKey::from_secret_key(sks[i])); wire.insert(wire.end(), pks[i].point.begin(), pks[i].point.end()); }
    mbls_keytable* kt = nullptr;
    CHECK(mbls_keytable_create(detail::ctx(), 4, &kt) == MBLS_OK);
    uint64_t first = 9; std::vector<uint8_t> errs(NK, 1);
    CHECK(mbls_keytable_append(kt, wire.data(), MBLS_PK_UNCOMPRESSED, 1, NK, &first, errs.data()) == MBLS_OK && first == 0);
    std::vector<Bytes> roots;
    for (int j = 0; j < 3; j++) roots.push_back(Bytes(32, uint8_t(0xD0 + j)));
    MessageTable table(1);
    CHECK(table.append(roots) == 0);
    {
        CommitteeTable committees(kt, 1);
        const std::vector<std::vector<uint32_t>> members = {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, {13, 12, 11}, {14, 15, 16, 17, 18, 19, 0, 1, 2}};
        CHECK(committees.append(members) == 0 && committees.max_members() == 11);
        using Set = CommitteeTable::GossipSet;
        // an aggregate of committee `id` by the members `sel` over entry `msg`; a signature of key `key` over entry `msg`
        std::vector<std::unique_ptr<AggregateSignature>> keep;
        auto aggregate = [&](uint32_t id, const std::vector<int>& sel, uint32_t msg) {
            keep.emplace_back(new AggregateSignature());
            Bytes f(members[id].size() / 8 + 1, 0);
            for (int j : sel) { f[j >> 3] |= uint8_t(1u << (j & 7)); keep.back()->add(Signature::new_(roots[msg], sks[members[id][j]])); }
            return Set::aggregate(keep.back().get(), id, f, msg);
        };
        auto single = [&](uint32_t key, uint32_t msg) {
            keep.emplace_back(new AggregateSignature());
            keep.back()->add(Signature::new_(roots[msg], sks[key]));
            return Set::single_key(keep.back().get(), key, msg);
        };
        const std::vector<Set> gossip = {aggregate(0, {0, 1, 2, 3, 4, 5, 6, 7, 8, 10}, 0), single(4, 1), single(17, 1), aggregate(2, {1, 8}, 1), single(9, 2), single(0, 0)};
        const std::vector<Set> singles = {single(3, 2), single(3, 0), single(19, 1)};
        std::vector<Set> wrong = {single(5, 0), aggregate(1, {0, 1, 2}, 2), single(6, 1)};
        wrong[1].bits[0] ^= 0x04;                                 // member 2 of committee 1 did sign, the field says it did not
        {
            VerifyMultipleStream vs(committees, table, 4, MBLS_STREAM_FULL_ROUNDS, 64);
            ByteRng rng(31), model(31);
            auto t1 = vs.submit(rng, gossip);
            auto t2 = vs.submit(rng, singles);
            auto t3 = vs.submit(rng, wrong);
            CHECK(!t1.ready());
            vs.flush();
            const auto want1 = committees.verify_multiple_aggregate_signatures_locate(model, gossip, table);
            const auto want2 = committees.verify_multiple_aggregate_signatures_locate(model, singles, table);
            const auto r1 = t1.get(); const auto r2 = t2.get(); const auto r3 = t3.get();
            CHECK(r1.first && want1.first && r1.second == want1.second && r1.second == std::vector<bool>(gossip.size(), true));
            CHECK(r2.first && want2.first && r2.second == want2.second);
            // the rejected batch: its own scalars (all of its signatures are in G2, so the method draws one per set as the stream did)
            const auto want3 = committees.verify_multiple_aggregate_signatures_locate(model, wrong, table);
            CHECK(!r3.first && !want3.first && r3.second == want3.second && r3.second == std::vector<bool>({true, false, true}));
            CHECK(rng.g == model.g);                              // one scalar per set, in set order, and nothing else
            const auto st3 = t3.status();
            CHECK((st3.second[1] & MBLS_ST_PAIRING_FAILED) && st3.second[0] == 0 && st3.second[2] == 0);
            CHECK(t1.status().first == 0 && t1.status().second == std::vector<uint32_t>(gossip.size(), 0));
            const mbls_stream_stats s = vs.stats();
            CHECK(s.calls == 3 && s.pieces == 3 && s.split_calls == 0 && s.items == 12 && s.rounds == 1);
            CHECK(s.gathered_bytes == 6 * (96 + 4 + 4 + 8 + 2) + 3 * (96 + 4 + 4 + 8 + 0) + 3 * (96 + 4 + 4 + 8 + 1));
            // what does not fit is refused: no sets, a field longer than the stride, a batch that costs more than a round
            for (int kind = 0; kind < 3; kind++) {
                bool threw = false;
                try {
                    std::vector<Set> b = kind == 0 ? std::vector<Set>() : kind == 1 ? wrong : std::vector<Set>(64, singles[0]);
                    if (kind == 1) b[1].bits = Bytes(5, 0);
                    (void)vs.submit(rng, b);
                } catch (const std::exception&) { threw = true; }
                CHECK(threw);
            }
            CHECK(vs.stats().calls == 3);
            bool threw = false;                                   // the table may not outgrow the stream's stride while the stream lives
            try { (void)committees.append({std::vector<uint32_t>(33, 0)}); } catch (const std::exception&) { threw = true; }
            CHECK(threw && committees.count() == 3);
        }
        CHECK(committees.append({std::vector<uint32_t>(33, 0)}) == 3);
    }
    mbls_keytable_destroy(kt);
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("all C++ verify_multiple stream checks passed\n");
    return 0;
}

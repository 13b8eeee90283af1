// CommitteeTable::verify_multiple_aggregate_signatures_batches[_locate] over SpanSet of include/milagro_bls.hpp
// (mbls_verify_multiple_batches_committee_span_msgtable[_locate]_rng): the nine sets of tests/cpp/test_vm_committee_span.cpp -- three attestations that span two
// committees, two committees and one committee, each followed by two sets under one key -- cut into four batches (one of them empty), one attestation with a wrong
// bit: one bool per batch, which set it is, and the generator left where AggregateSignature::verify_multiple_aggregate_signatures_batches on the spelled-out keys
// and messages leaves it. Exit code 0 = all passed.
#include <cstdio>
#include <cstdlib>
#include <random>
#include "milagro_bls.hpp"
using namespace milagro_bls;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); fails++; } } while (0)
typedef std::tuple<const AggregateSignature*, const AggregatePublicKey*, Bytes> Set;
typedef CommitteeTable::SpanSet G;

int main() {
    std::mt19937 gen(23);
    auto rand_sk = [&] { Bytes b(32); for (auto& v : b) v = uint8_t(gen()); b[0] &= 0x3f; b[31] |= 1; return SecretKey::from_bytes(b); };
    const int NK = 12;
    std::vector<SecretKey> sks; std::vector<PublicKey> pks; Bytes wire;
    for (int i = 0; i < NK; i++) { sks.push_back(rand_sk()); pks.push_back(PublicKey::from_secret_key(sks[i])); wire.insert(wire.end(), pks[i].point.begin(), pks[i].point.end()); }
    mbls_keytable* kt = nullptr;
    CHECK(mbls_keytable_create(detail::ctx(), 4, &kt) == MBLS_OK);
    uint64_t first = 9; std::vector<uint8_t> errs(NK, 1);
    CHECK(mbls_keytable_append(kt, wire.data(), MBLS_PK_UNCOMPRESSED, 1, NK, &first, errs.data()) == MBLS_OK && first == 0);
    std::vector<Bytes> roots;
    for (int j = 0; j < 4; j++) roots.push_back(Bytes(32, uint8_t(0xC0 + j)));
    MessageTable table(1);
    CHECK(table.append(roots) == 0);
    {
        CommitteeTable committees(kt, 1);
        const std::vector<std::vector<uint32_t>> members = {{0, 1, 2, 3, 4, 5, 6, 7, 8}, {11, 10, 9}, {3, 7}};
        CHECK(committees.append(members) == 0 && committees.count() == 3 && committees.max_members() == 9);
        // attestations, by position in the concatenated members: committees 0 + 1 (12 bits) without member 4 of committee 0 (complement route) and with committee 1
        // in full; committees 2 + 0 (11 bits) with member 1 of committee 2 and members 1 and 8 of committee 0; committee 1 alone in full with a delimiter bit above
        const std::vector<std::vector<uint32_t>> cids = {{0, 1}, {2, 0}, {1}};
        const std::vector<std::vector<int>> sel = {{0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11}, {1, 3, 10}, {0, 1, 2}};
        const uint32_t msg[3] = {0, 3, 1};
        std::vector<Bytes> bits = {Bytes{0xEF, 0x0F}, Bytes{0x0A, 0x04}, Bytes{0x0F}};
        std::vector<AggregateSignature> sigs(9); std::vector<AggregatePublicKey> apks(9); std::vector<uint32_t> midx(9), single(9);
        for (int a = 0; a < 3; a++) {
            const int i = 3 * a;
            midx[i] = msg[a];
            for (size_t t = 0; t < sel[a].size(); t++) {
                std::vector<uint32_t> all;                                               // the span's members, concatenated
                for (uint32_t c : cids[a]) all.insert(all.end(), members[c].begin(), members[c].end());
                const uint32_t key = all[sel[a][t]];
                sigs[i].add(Signature::new_(roots[msg[a]], sks[key]));
                if (t == 0) apks[i] = AggregatePublicKey::from_public_key(pks[key]); else apks[i].add(pks[key]);
            }
            for (int q = 1; q <= 2; q++) {                                                  // the selection proof and the aggregator's signature: one key each
                single[i + q] = uint32_t((5 * a + q) % NK); midx[i + q] = uint32_t((a + q) % 4);
                sigs[i + q].add(Signature::new_(roots[midx[i + q]], sks[single[i + q]]));
                apks[i + q] = AggregatePublicKey::from_public_key(pks[single[i + q]]);
            }
        }
        const size_t cuts[5] = {0, 2, 2, 6, 9};                                                // batch 1 is empty; set 3, the bent one, lies in batch 2
        auto gossip = [&](bool bad) {
            std::vector<G> v;
            for (int a = 0; a < 3; a++) {
                Bytes b = bits[a];
                if (bad && a == 1) b[0] |= 0x80;                                            // position 7 = member 5 of committee 0 did not sign
                v.push_back(G::attestation(&sigs[3 * a], cids[a], b, midx[3 * a]));
                for (int q = 1; q <= 2; q++) v.push_back(G::single_key(&sigs[3 * a + q], single[3 * a + q], midx[3 * a + q]));
            }
            std::vector<std::vector<G>> out;
            for (int b = 0; b < 4; b++) out.emplace_back(v.begin() + cuts[b], v.begin() + cuts[b + 1]);
            return out;
        };
        AggregatePublicKey wrong = apks[3]; wrong.add(pks[5]);
        auto spelled = [&](bool bad) {
            std::vector<std::vector<Set>> out(4);
            for (int b = 0; b < 4; b++)
                for (size_t i = cuts[b]; i < cuts[b + 1]; i++) out[b].emplace_back(&sigs[i], bad && i == 3 ? &wrong : &apks[i], roots[midx[i]]);
            return out;
        };
        std::mt19937 g1(5), g2(5), g3(5);
        auto r1 = [&] { return uint8_t(g1()); };
        auto r2 = [&] { return uint8_t(g2()); };
        auto r3 = [&] { return uint8_t(g3()); };
        const std::vector<bool> all(4, true), one_bad = {true, true, false, true};
        CHECK(committees.verify_multiple_aggregate_signatures_batches(r1, gossip(false), table) == all);
        CHECK(committees.verify_multiple_aggregate_signatures_batches(r1, gossip(true), table) == one_bad);
        auto good = committees.verify_multiple_aggregate_signatures_batches_locate(r2, gossip(false), table);
        CHECK(good.first == all && good.second.size() == 4 && good.second[1].empty() && good.second[2] == std::vector<bool>(4, true));
        auto got = committees.verify_multiple_aggregate_signatures_batches_locate(r2, gossip(true), table);
        const std::vector<bool> want2 = {true, false, true, true};
        CHECK(got.first == one_bad && got.second[0] == std::vector<bool>(2, true) && got.second[2] == want2 && got.second[3] == std::vector<bool>(3, true));
        // the batches method on the spelled-out keys and messages, a generator with the same seed: same bools, same generator state afterwards
        CHECK(AggregateSignature::verify_multiple_aggregate_signatures_batches(r3, spelled(false)) == all);
        CHECK(AggregateSignature::verify_multiple_aggregate_signatures_batches(r3, spelled(true)) == one_bad);
        const auto a = g1(), b = g2(), c = g3();
        CHECK(a == b && b == c);
        // what names nothing is refused, no batches answer nothing
        for (int kind = 0; kind < 5; kind++) {
            bool threw = false;
            try {
                auto v = gossip(false);
                if (kind == 0) v[0][0].committee_ids[1] = 3; else if (kind == 1) v[0][1].committee_ids[0] = MBLS_VM_SET_SINGLE_KEY | NK; else if (kind == 2) v[2][0].msg_index = 4;
                else if (kind == 3) v[0][0].committee_ids.push_back(MBLS_VM_SET_SINGLE_KEY | 1); else v[0][0].committee_ids.assign(65, 0);      // more than MBLS_SPAN_MAX_COMMITTEES ids
                (void)committees.verify_multiple_aggregate_signatures_batches(r1, v, table);
            } catch (const std::exception&) { threw = true; }
            CHECK(threw);
        }
        CHECK(committees.verify_multiple_aggregate_signatures_batches(r1, std::vector<std::vector<G>>(), table).empty());
        // (a braced list keeps naming the GossipSet overloads)
        CHECK(committees.verify_multiple_aggregate_signatures_batches(r1, {}, table).empty());
    }
    mbls_keytable_destroy(kt);
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("all C++ verify_multiple batches committee span checks passed\n");
    return 0;
}

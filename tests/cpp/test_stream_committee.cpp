// VerifyStream over a CommitteeTable and a MessageTable of include/milagro_bls.hpp (mbls_stream_create_committee, mbls_stream_submit_committee): one mixed call --
// nearly everybody signing (the complement route), a few signing (the direct route), nobody, a Bitlist's delimiter left in, one wrong bit, a committee id and an
// entry index that name nothing -- gives the bools of AggregateSignature::fast_aggregate_verify on the members spelled out; a second call carries shorter fields.
// Exit code 0 = all passed.
#include <cstdio>
#include <cstdlib>
#include <random>
#include "milagro_bls.hpp"
using namespace milagro_bls;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); fails++; } } while (0)

int main() {
    std::mt19937 gen(7251);
    auto rand_sk = [&] { Bytes b(32); for (auto& v : b) v = uint8_t(gen()); b[0] &= 0x3f; b[31] |= 1; return SecretKey::from_bytes(b); };
    const int NK = 20;
    std::vector<SecretKey> sks; std::vector<PublicKey> pks; Bytes wire;
    for (int i = 0; i < NK; i++) { sks.push_back(rand_sk()); pks.push_back(PublicKey::from_secret_key(sks[i])); wire.insert(wire.end(), pks[i].point.begin(), pks[i].point.end()); }
    mbls_keytable* kt = nullptr;
    CHECK(mbls_keytable_create(detail::ctx(), 4, &kt) == MBLS_OK);
    uint64_t first = 9; std::vector<uint8_t> errs(NK, 1);
    CHECK(mbls_keytable_append(kt, wire.data(), MBLS_PK_UNCOMPRESSED, 1, NK, &first, errs.data()) == MBLS_OK && first == 0);
    std::vector<Bytes> roots;
    for (int j = 0; j < 3; j++) roots.push_back(Bytes(32, uint8_t(0xC0 + j)));
    MessageTable table(1);
    CHECK(table.append(roots) == 0);
    {
        CommitteeTable committees(kt, 1);
        const std::vector<std::vector<uint32_t>> members = {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, {13, 12, 11}, {14, 15, 16, 17, 18, 19, 0, 1, 2}};
        CHECK(committees.append(members) == 0 && committees.count() == 3 && committees.max_members() == 11);
        struct Att { uint32_t id; std::vector<int> sel; uint32_t msg; };
        const std::vector<Att> atts = {
            {0, {0, 1, 2, 3, 4, 5, 6, 7, 8, 10}, 0},          // all but member 9: complement
            {2, {1, 8}, 1},                                    // two of nine: direct
            {1, {0, 1, 2}, 2},                                 // everybody
            {1, {}, 0},                                        // nobody: no keys
            {2, {0, 1, 2, 3, 4, 5, 6, 7}, 2}};                 // eight of nine: the field's first byte is full
        std::vector<AggregateSignature> sigs(atts.size()); std::vector<Bytes> fields; std::vector<std::vector<const PublicKey*>> spelled(atts.size());
        std::vector<uint32_t> ids, idx;
        for (size_t a = 0; a < atts.size(); a++) {
            const size_t m = members[atts[a].id].size();
            Bytes f(m / 8 + 1, 0);
            for (int j : atts[a].sel) {
                const uint32_t key = members[atts[a].id][j];
                f[j >> 3] |= uint8_t(1u << (j & 7));
                sigs[a].add(Signature::new_(roots[atts[a].msg], sks[key]));
                spelled[a].push_back(&pks[key]);
            }
            f[m >> 3] |= uint8_t(1u << (m & 7));                // the Bitlist's delimiter stays
            fields.push_back(f); ids.push_back(atts[a].id); idx.push_back(atts[a].msg);
        }
        if (atts[3].sel.empty()) sigs[3] = sigs[2];             // (some signature: the item has no keys)
        {
            VerifyStream vs(committees, table, 4, MBLS_STREAM_FULL_ROUNDS, 256);
            std::vector<uint32_t> st;
            auto t1 = vs.submit_committee(sigs, idx, ids, fields, &st);          // fields of 1 and 2 bytes travel as 2
            auto bad_fields = fields; bad_fields[1][0] ^= 0x08;                   // member 3 of committee 2 did not sign
            auto bad_ids = ids; bad_ids[0] = 3;                                   // no such committee
            auto bad_idx = idx; bad_idx[2] = 3;                                   // no such entry
            auto t2 = vs.submit_committee(sigs, idx, ids, bad_fields);
            auto t3 = vs.submit_committee(sigs, bad_idx, bad_ids, fields);
            // shorter fields in a call of their own: items 1 and 2 alone travel at 1 byte where committee 2's delimiter (bit 9) is cut off
            std::vector<AggregateSignature> s2 = {sigs[2], sigs[4]};
            auto t4 = vs.submit_committee(s2, {idx[2], idx[4]}, {ids[2], ids[4]}, {Bytes(1, fields[2][0]), Bytes(1, fields[4][0])});
            CHECK(!t1.ready());
            vs.flush();
            const auto good = t1.get();
            CHECK(good.size() == atts.size());
            for (size_t a = 0; a < atts.size(); a++) {
                const bool want = !spelled[a].empty() && sigs[a].fast_aggregate_verify(roots[atts[a].msg], spelled[a]);
                CHECK(good[a] == want);
                CHECK(good[a] == (a != 3));
            }
            CHECK(st.size() == atts.size() && st[0] == 0 && st[1] == 0 && st[2] == 0 && (st[3] & MBLS_ST_NO_KEYS) && st[4] == 0);
            const auto bad = t2.get();
            for (size_t a = 0; a < atts.size(); a++) CHECK(bad[a] == (a != 1 && a != 3));
            const auto named = t3.get();
            for (size_t a = 0; a < atts.size(); a++) CHECK(named[a] == (a == 1 || a == 4));
            const auto shorter = t4.get();
            CHECK(shorter.size() == 2 && shorter[0] && shorter[1]);
            const mbls_stream_stats s = vs.stats();
            CHECK(s.calls == 4 && s.items == 17 && s.rounds == 1);
            CHECK(s.gathered_bytes == 15 * (96 + 4 + 4 + 2) + 2 * (96 + 4 + 4 + 1));
            // what does not fit is refused: a field longer than the stride, lists of different lengths
            for (int kind = 0; kind < 2; kind++) {
                bool threw = false;
                try {
                    auto f = fields; auto i2 = idx;
                    if (kind == 0) f[0] = Bytes(5, 0); else i2.pop_back();
                    (void)vs.submit_committee(sigs, i2, ids, f);
                } catch (const std::exception&) { threw = true; }
                CHECK(threw);
            }
            // the table may not outgrow the stream's stride while the stream lives
            bool threw = false;
            try { (void)committees.append({std::vector<uint32_t>(33, 0)}); } catch (const std::exception&) { threw = true; }
            CHECK(threw && committees.count() == 3);
        }
        CHECK(committees.append({std::vector<uint32_t>(33, 0)}) == 3);
        bool threw = false;
        try { VerifyStream vs(committees, table, 4); } catch (const std::exception&) { threw = true; }       // 32 bits no longer cover the table
        CHECK(threw);
    }
    mbls_keytable_destroy(kt);
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("all C++ committee stream checks passed\n");
    return 0;
}

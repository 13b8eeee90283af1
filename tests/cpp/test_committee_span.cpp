// CommitteeTable::fast_aggregate_verify_spans of include/milagro_bls.hpp (mbls_fast_aggregate_verify_batch_committee_span_msgtable): attestations over two and
// three committees of a table of four -- nearly everybody signing (the complement route), a few signing (the direct route), a segment with nobody beside one with
// signers, a delimiter bit left in, an empty span --, and one attestation with a wrong bit: the bools of AggregateSignature::fast_aggregate_verify on the members
// spelled out. What names nothing throws.
// Exit code 0 = all passed.
#include <cstdio>
#include <cstdlib>
#include <random>
#include "milagro_bls.hpp"
using namespace milagro_bls;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); fails++; } } while (0)
typedef CommitteeTable::SpanItem S;

int main() {
    std::mt19937 gen(7549);
    auto rand_sk = [&] { Bytes b(32); for (auto& v : b) v = uint8_t(gen()); b[0] &= 0x3f; b[31] |= 1; return SecretKey::from_bytes(b); };
    const int NK = 24;
    std::vector<SecretKey> sks; std::vector<PublicKey> pks; Bytes wire;
    for (int i = 0; i < NK; i++) { sks.push_back(rand_sk()); pks.push_back(PublicKey::from_secret_key(sks[i])); wire.insert(wire.end(), pks[i].point.begin(), pks[i].point.end()); }
    mbls_keytable* kt = nullptr;
    CHECK(mbls_keytable_create(detail::ctx(), 4, &kt) == MBLS_OK);
    uint64_t first = 9; std::vector<uint8_t> errs(NK, 1);
    CHECK(mbls_keytable_append(kt, wire.data(), MBLS_PK_UNCOMPRESSED, 1, NK, &first, errs.data()) == MBLS_OK && first == 0);
    std::vector<Bytes> roots;
    for (int j = 0; j < 3; j++) roots.push_back(Bytes(32, uint8_t(0xE0 + j)));
    MessageTable table(1);
    CHECK(table.append(roots) == 0);
    {
        CommitteeTable committees(kt, 1);
        const std::vector<std::vector<uint32_t>> members = {{0, 1, 2, 3, 4, 5, 6, 7, 8}, {11, 10, 9}, {12, 13, 14, 15, 16, 17, 18}, {23, 22, 21, 20, 19}};
        CHECK(committees.append(members) == 0 && committees.count() == 4);
        // an attestation: its committees and, per committee, the member positions that signed
        struct Att { std::vector<uint32_t> ids; std::vector<std::vector<int>> sel; uint32_t msg; };
        const std::vector<Att> atts = {
            {{0, 1}, {{0, 1, 2, 3, 5, 6, 7, 8}, {0, 1, 2}}, 0},                    // committee 0 without member 4, committee 1 in full: both complement
            {{2, 0, 3}, {{1}, {0, 1, 2, 3, 4, 5, 6, 7, 8}, {4}}, 1},              // direct, complement, direct
            {{1, 2}, {{}, {0, 1, 2, 3, 4, 5}}, 2},                                // nobody beside signers
            {{3, 3}, {{0, 1, 2, 3, 4}, {0, 1, 2, 3, 4}}, 0},                      // the same committee twice
            {{}, {}, 1}};                                                         // no committee: no keys
        std::vector<AggregateSignature> sigs(atts.size()); std::vector<Bytes> fields; std::vector<std::vector<const PublicKey*>> spelled(atts.size());
        for (size_t a = 0; a < atts.size(); a++) {
            size_t o = 0, M = 0;
            for (uint32_t id : atts[a].ids) M += members[id].size();
            Bytes f(M / 8 + 1, 0);
            for (size_t t = 0; t < atts[a].ids.size(); t++) {
                for (int j : atts[a].sel[t]) {
                    const uint32_t key = members[atts[a].ids[t]][j];
                    f[(o + j) >> 3] |= uint8_t(1u << ((o + j) & 7));
                    sigs[a].add(Signature::new_(roots[atts[a].msg], sks[key]));
                    spelled[a].push_back(&pks[key]);
                }
                o += members[atts[a].ids[t]].size();
            }
            f[M >> 3] |= uint8_t(1u << (M & 7));                                   // the Bitlist's delimiter stays
            fields.push_back(f);
        }
        auto items = [&](bool bad) {
            std::vector<S> v;
            for (size_t a = 0; a < atts.size(); a++) {
                Bytes f = fields[a];
                if (bad && a == 1) f[0] ^= 0x04;                                   // member 2 of committee 2 did not sign
                v.push_back(S{&sigs[a], atts[a].ids, f, atts[a].msg});
            }
            return v;
        };
        std::vector<uint32_t> st;
        const auto good = committees.fast_aggregate_verify_spans(items(false), table, &st);
        CHECK(good.size() == atts.size());
        for (size_t a = 0; a < atts.size(); a++) {
            const bool want = !spelled[a].empty() && sigs[a].fast_aggregate_verify(roots[atts[a].msg], spelled[a]);
            CHECK(good[a] == want);
            CHECK(good[a] == (a != 4));
        }
        CHECK(st.size() == atts.size() && st[0] == 0 && st[1] == 0 && st[2] == 0 && st[3] == 0 && (st[4] & MBLS_ST_NO_KEYS));
        const auto bad = committees.fast_aggregate_verify_spans(items(true), table);
        for (size_t a = 0; a < atts.size(); a++) CHECK(bad[a] == (a != 1 && a != 4));
        // what names nothing or does not fit is refused, an empty batch accepts
        for (int kind = 0; kind < 4; kind++) {
            bool threw = false;
            try {
                auto v = items(false);
                if (kind == 0) v[0].committee_ids[1] = 4;
                else if (kind == 1) v[1].msg_index = 3;
                else if (kind == 2) v[2].committee_ids.assign(65, 1);
                else v[0].committee_ids.assign(4, 0);                               // the widest field has 3 bytes (a stride of 4): 32 bits do not cover 36 members
                (void)committees.fast_aggregate_verify_spans(v, table);
            } catch (const std::exception&) { threw = true; }
            CHECK(threw);
        }
        CHECK(committees.fast_aggregate_verify_spans({}, table).empty());
    }
    mbls_keytable_destroy(kt);
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("all C++ committee span checks passed\n");
    return 0;
}

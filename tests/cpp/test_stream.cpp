// milagro_bls::VerifyStream (include/milagro_bls.hpp) over the reference's own test shapes (src/aggregates.rs:384-530: an empty key list, keys
// summing to infinity, an aggregate of four signers, its subset and superset, a wrong message), packed with random valid and invalid items into
// calls of uneven size; every item is checked against the scalar API. Exit code 0 = all passed.
#include <cstdio>
#include <random>
#include "milagro_bls.hpp"
using namespace milagro_bls;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); fails++; } } while (0)
static Bytes str(const char* s) { return Bytes(s, s + std::strlen(s)); }

int main() {
    std::mt19937 gen(11);
    auto rand_sk = [&] { Bytes b(32); for (auto& v : b) v = uint8_t(gen()); b[0] &= 0x3f; b[31] |= 1; return SecretKey::from_bytes(b); };
    std::vector<Keypair> kps; for (int i = 0; i < 6; i++) { SecretKey s = rand_sk(); kps.push_back(Keypair{s, PublicKey::from_secret_key(s)}); }
    Bytes one(32, 0); one[31] = 1;
    static PublicKey p1 = PublicKey::from_secret_key(SecretKey::from_bytes(one));
    static PublicKey pm = PublicKey::from_secret_key(SecretKey::from_bytes(Bytes{0x73, 0xed, 0xa7, 0x53, 0x29, 0x9d, 0x7d, 0x48, 0x33, 0x39, 0xd8, 0x08, 0x09, 0xa1, 0xd8, 0x05,
                                                                               0x53, 0xbd, 0xa4, 0x02, 0xff, 0xfe, 0x5b, 0xfe, 0xff, 0xff, 0xff, 0xff, 0x00, 0x00, 0x00, 0x00}));
    struct Item { AggregateSignature sig; Bytes msg; std::vector<const PublicKey*> keys; };
    std::vector<Item> items;
    items.push_back({AggregateSignature(), Bytes(32, 0), {}});                                 // empty key list
    items.push_back({AggregateSignature(), Bytes(32, 0), {&p1, &pm}});                         // keys summing to infinity
    for (int r = 0; r < 40; r++) {
        Bytes msg = str("Small msg"); msg.push_back(uint8_t(r)); if (r % 5 == 0) msg.resize(msg.size() + r);   // messages of several lengths
        const int m = 1 + r % 6;
        AggregateSignature agg; std::vector<const PublicKey*> pks;
        for (int i = 0; i < m; i++) { agg.add(Signature::new_(msg, kps[i].sk)); pks.push_back(&kps[i].pk); }
        items.push_back({agg, msg, pks});                                                       // valid
        if (m > 1) { auto sub = pks; sub.pop_back(); items.push_back({agg, msg, sub}); }      // subset
        { AggregateSignature dbl = agg; dbl.add(Signature::new_(msg, kps[0].sk)); items.push_back({dbl, msg, pks}); }   // superset
        { Bytes other = msg; other[0] ^= 1; items.push_back({agg, other, pks}); }              // wrong message
    }
    std::vector<bool> want;
    for (auto& it : items) want.push_back(it.sig.fast_aggregate_verify(it.msg, it.keys));
    for (uint32_t policy : {uint32_t(MBLS_STREAM_WORK_CONSERVING), uint32_t(MBLS_STREAM_FULL_ROUNDS)}) {
        VerifyStream vs(policy, 64);                                                            // small rounds: calls are split
        std::vector<std::pair<size_t, VerifyStream::Ticket>> ts;
        for (size_t a = 0; a < items.size();) {
            const size_t n = std::min(items.size() - a, size_t(1 + gen() % 50));
            std::vector<AggregateSignature> s; std::vector<Bytes> m; std::vector<std::vector<const PublicKey*>> k;
            for (size_t i = a; i < a + n; i++) { s.push_back(items[i].sig); m.push_back(items[i].msg); k.push_back(items[i].keys); }
            ts.emplace_back(a, vs.submit(s, m, k));
            a += n;
        }
        vs.flush();
        for (auto& [a, t] : ts) {
            std::vector<bool> got = t.get();
            for (size_t i = 0; i < got.size(); i++) CHECK(got[i] == want[a + i]);
            CHECK(t.ready());
        }
        mbls_stream_stats st = vs.stats();
        CHECK(st.calls == ts.size() && st.items == items.size() && st.rounds >= (items.size() + 63) / 64);
    }
    CHECK(!want[0] && !want[1] && want[2]);
    if (fails) { std::printf("%d C++ stream checks failed\n", fails); return 1; }
    std::printf("all C++ stream checks passed (%zu items)\n", items.size());
    return 0;
}

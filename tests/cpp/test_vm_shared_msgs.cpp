// AggregateSignature::verify_multiple_aggregate_signatures_shared_msgs of include/milagro_bls.hpp (mbls_verify_multiple_shared_msgs_rng): eight sets over three
// messages give the bool of verify_multiple_aggregate_signatures and leave the generator where it leaves it -- valid, and with the message of the first, a
// middle and the last set changed. Exit code 0 = all passed.
#include <cstdio>
#include <cstdlib>
#include <random>
#include "milagro_bls.hpp"
using namespace milagro_bls;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); fails++; } } while (0)

int main() {
    std::mt19937 gen(29);
    auto rand_sk = [&] { Bytes b(32); for (auto& v : b) v = uint8_t(gen()); b[0] &= 0x3f; b[31] |= 1; return SecretKey::from_bytes(b); };
    const std::vector<Bytes> msgs = {Bytes(32, 1), Bytes(7, 2), Bytes()};           // messages of any length each, the empty one included
    const int n = 8;
    const int which[n] = {0, 1, 0, 2, 1, 0, 0, 2};
    std::vector<AggregateSignature> sigs(n); std::vector<AggregatePublicKey> apks(n);
    for (int i = 0; i < n; i++) {
        std::vector<PublicKey> pks;
        for (int j = 0; j < 2; j++) { SecretKey sk = rand_sk(); sigs[i].add(Signature::new_(msgs[which[i]], sk)); pks.push_back(PublicKey::from_secret_key(sk)); }
        apks[i] = AggregatePublicKey::into_aggregate(pks);
    }
    typedef std::vector<std::tuple<const AggregateSignature*, const AggregatePublicKey*, Bytes>> Sets;
    auto sets_of = [&](int changed) { Sets s; for (int i = 0; i < n; i++) s.emplace_back(&sigs[i], &apks[i], i == changed ? Bytes(5, 9) : msgs[which[i]]); return s; };
    for (int changed : {-1, 0, 4, 7}) {
        Sets sets = sets_of(changed);
        std::mt19937 g1(77), g2(77);
        auto r1 = [&] { return uint8_t(g1()); }; auto r2 = [&] { return uint8_t(g2()); };
        const bool want = AggregateSignature::verify_multiple_aggregate_signatures(r1, sets);
        const bool got = AggregateSignature::verify_multiple_aggregate_signatures_shared_msgs(r2, sets);
        CHECK(want == (changed < 0));
        CHECK(got == want);
        CHECK(g1() == g2());                                                        // as many bytes drawn
    }
    std::mt19937 g0(1);
    auto r0 = [&] { return uint8_t(g0()); };
    CHECK(AggregateSignature::verify_multiple_aggregate_signatures_shared_msgs(r0, Sets()));
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("all C++ shared message verify_multiple checks passed\n");
    return 0;
}

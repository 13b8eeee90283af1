// AggregateSignature::verify_multiple_aggregate_signatures_shared_msgs_locate of include/milagro_bls.hpp (mbls_verify_multiple_shared_msgs_locate_rng): nine
// sets over three messages, one of them bad -- the bool, which set it is, and the generator left where the shared-message method leaves it. Exit code 0 = all
// passed.
#include <cstdio>
#include <cstdlib>
#include <random>
#include "milagro_bls.hpp"
using namespace milagro_bls;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); fails++; } } while (0)
typedef std::tuple<const AggregateSignature*, const AggregatePublicKey*, Bytes> Set;

int main() {
    std::mt19937 gen(13);
    auto rand_sk = [&] { Bytes b(32); for (auto& v : b) v = uint8_t(gen()); b[0] &= 0x3f; b[31] |= 1; return SecretKey::from_bytes(b); };
    std::vector<Bytes> roots;
    for (int j = 0; j < 3; j++) roots.push_back(Bytes(32 + j, uint8_t(0xA0 + j)));
    std::vector<SecretKey> sks; std::vector<AggregateSignature> sigs(9); std::vector<AggregatePublicKey> apks;
    for (int i = 0; i < 9; i++) {
        sks.push_back(rand_sk());
        sigs[i].add(Signature::new_(roots[i % 3], sks[i]));
        apks.push_back(AggregatePublicKey::from_public_key(PublicKey::from_secret_key(sks[i])));
    }
    AggregateSignature wrong; wrong.add(Signature::new_(roots[4 % 3], sks[5]));     // set 4 signed with set 5's key
    auto sets = [&](bool bad) {
        std::vector<Set> v;
        for (int i = 0; i < 9; i++) v.emplace_back(bad && i == 4 ? &wrong : &sigs[i], &apks[i], roots[i % 3]);
        return v;
    };
    std::mt19937 g1(5), g2(5);
    auto r1 = [&] { return uint8_t(g1()); };
    auto r2 = [&] { return uint8_t(g2()); };
    auto good = AggregateSignature::verify_multiple_aggregate_signatures_shared_msgs_locate(r1, sets(false));
    CHECK(good.first && good.second == std::vector<bool>(9, true));
    auto got = AggregateSignature::verify_multiple_aggregate_signatures_shared_msgs_locate(r1, sets(true));
    std::vector<bool> want(9, true); want[4] = false;
    CHECK(!got.first && got.second == want);
    // the shared-message method on a generator with the same seed: same bools, same generator state afterwards
    CHECK(AggregateSignature::verify_multiple_aggregate_signatures_shared_msgs(r2, sets(false)) == good.first);
    CHECK(AggregateSignature::verify_multiple_aggregate_signatures_shared_msgs(r2, sets(true)) == got.first);
    CHECK(g1() == g2());
    { auto e = AggregateSignature::verify_multiple_aggregate_signatures_shared_msgs_locate(r1, {}); CHECK(e.first && e.second.empty()); }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("all C++ shared-message locate checks passed\n");
    return 0;
}

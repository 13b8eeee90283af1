// AggregateSignature::verify_multiple_aggregate_signatures_batches_locate of include/milagro_bls.hpp (mbls_verify_multiple_batches_locate_rng): three batches, the
// middle one with one bad set -- the per-batch bools, which set it is, and the generator left where the batches method leaves it. Exit code 0 = all passed.
#include <cstdio>
#include <cstdlib>
#include <random>
#include "milagro_bls.hpp"
using namespace milagro_bls;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); fails++; } } while (0)
typedef std::tuple<const AggregateSignature*, const AggregatePublicKey*, Bytes> Set;

int main() {
    std::mt19937 gen(12);
    auto rand_sk = [&] { Bytes b(32); for (auto& v : b) v = uint8_t(gen()); b[0] &= 0x3f; b[31] |= 1; return SecretKey::from_bytes(b); };
    const int sizes[3] = {3, 4, 2};
    std::vector<SecretKey> sks; std::vector<AggregateSignature> sigs(9); std::vector<AggregatePublicKey> apks; std::vector<Bytes> msgs;
    for (int i = 0; i < 9; i++) {
        sks.push_back(rand_sk());
        msgs.push_back(Bytes(20 + 3 * i, uint8_t(i)));
        sigs[i].add(Signature::new_(msgs[i], sks[i]));
        apks.push_back(AggregatePublicKey::from_public_key(PublicKey::from_secret_key(sks[i])));
    }
    AggregateSignature wrong; wrong.add(Signature::new_(msgs[4], sks[5]));     // set 4 (batch 1, its second set) signed with set 5's key
    auto cut = [&](bool bad) {
        std::vector<std::vector<Set>> batches(3);
        for (int b = 0, i = 0; b < 3; b++) for (int j = 0; j < sizes[b]; j++, i++) batches[b].emplace_back(bad && i == 4 ? &wrong : &sigs[i], &apks[i], msgs[i]);
        return batches;
    };
    std::mt19937 g1(5), g2(5);
    auto r1 = [&] { return uint8_t(g1()); };
    auto r2 = [&] { return uint8_t(g2()); };
    auto good = AggregateSignature::verify_multiple_aggregate_signatures_batches_locate(r1, cut(false));
    CHECK(good.first == std::vector<bool>({true, true, true}));
    CHECK(good.second.size() == 3 && good.second[0] == std::vector<bool>(3, true) && good.second[1] == std::vector<bool>(4, true) && good.second[2] == std::vector<bool>(2, true));
    auto got = AggregateSignature::verify_multiple_aggregate_signatures_batches_locate(r1, cut(true));
    CHECK(got.first == std::vector<bool>({true, false, true}));
    CHECK(got.second.size() == 3 && got.second[0] == std::vector<bool>(3, true) && got.second[1] == std::vector<bool>({true, false, true, true}) &&
          got.second[2] == std::vector<bool>(2, true));
    // the batches method on a generator with the same seed: same bools, same generator state afterwards
    CHECK(AggregateSignature::verify_multiple_aggregate_signatures_batches(r2, cut(false)) == good.first);
    CHECK(AggregateSignature::verify_multiple_aggregate_signatures_batches(r2, cut(true)) == got.first);
    CHECK(g1() == g2());
    { auto e = AggregateSignature::verify_multiple_aggregate_signatures_batches_locate(r1, {}); CHECK(e.first.empty() && e.second.empty()); }
    { auto e = AggregateSignature::verify_multiple_aggregate_signatures_batches_locate(r1, std::vector<std::vector<Set>>(2));
      CHECK(e.first == std::vector<bool>(2, true) && e.second.size() == 2 && e.second[0].empty() && e.second[1].empty()); }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("all C++ verify_multiple locate checks passed\n");
    return 0;
}

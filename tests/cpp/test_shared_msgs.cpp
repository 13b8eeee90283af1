// fast_aggregate_verify_batch_shared_msgs of include/milagro_bls.hpp (mbls_fast_aggregate_verify_batch_shared_msgs): six items over a list of three messages,
// one of them with an index that names another message than its signers saw -- the same bools as one fast_aggregate_verify per item. Exit code 0 = all passed.
#include <cstdio>
#include <cstdlib>
#include <random>
#include "milagro_bls.hpp"
using namespace milagro_bls;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); fails++; } } while (0)

int main() {
    std::mt19937 gen(23);
    auto rand_sk = [&] { Bytes b(32); for (auto& v : b) v = uint8_t(gen()); b[0] &= 0x3f; b[31] |= 1; return SecretKey::from_bytes(b); };
    const std::vector<Bytes> msgs = {Bytes(32, 1), Bytes(7, 2), Bytes(64, 3)};      // messages of any length each
    const int n = 6;
    std::vector<uint32_t> idx = {2, 1, 0, 1, 2, 0};                                 // item 0 names message 2, item 2 names message 0
    std::vector<SecretKey> sks; std::vector<PublicKey> pks;
    for (int i = 0; i < 2 * n; i++) { sks.push_back(rand_sk()); pks.push_back(PublicKey::from_secret_key(sks.back())); }
    std::vector<AggregateSignature> sigs(n); std::vector<std::vector<const PublicKey*>> keys(n);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 2; j++) { sigs[i].add(Signature::new_(msgs[idx[i]], sks[2 * i + j])); keys[i].push_back(&pks[2 * i + j]); }
    auto good = fast_aggregate_verify_batch_shared_msgs(sigs, msgs, idx, keys);
    CHECK(good.size() == size_t(n));
    for (int i = 0; i < n; i++) CHECK(good[i] && sigs[i].fast_aggregate_verify(msgs[idx[i]], keys[i]));
    idx[3] = 0;                                                                     // signed over message 1, names message 0
    auto got = fast_aggregate_verify_batch_shared_msgs(sigs, msgs, idx, keys);
    for (int i = 0; i < n; i++) CHECK(got[i] == (i != 3));
    CHECK(!sigs[3].fast_aggregate_verify(msgs[0], keys[3]));
    idx[3] = 3;                                                                     // names no message: refused before anything runs
    bool threw = false;
    try { fast_aggregate_verify_batch_shared_msgs(sigs, msgs, idx, keys); } catch (const std::invalid_argument&) { threw = true; }
    CHECK(threw);
    CHECK(fast_aggregate_verify_batch_shared_msgs({}, msgs, {}, {}).empty());
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("all C++ shared message list checks passed\n");
    return 0;
}

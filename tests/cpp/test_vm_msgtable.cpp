// MessageTable::verify_multiple_aggregate_signatures[_locate] of include/milagro_bls.hpp (mbls_verify_multiple_msgtable[_locate]_rng): nine sets naming three
// of five entries of a resident table, one of them bad -- the bool, which set it is, and the generator left where verify_multiple_aggregate_signatures on the
// spelled-out messages leaves it. Exit code 0 = all passed.
#include <cstdio>
#include <cstdlib>
#include <random>
#include "milagro_bls.hpp"
using namespace milagro_bls;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); fails++; } } while (0)
typedef std::tuple<const AggregateSignature*, const AggregatePublicKey*, Bytes> Set;

int main() {
    std::mt19937 gen(17);
    auto rand_sk = [&] { Bytes b(32); for (auto& v : b) v = uint8_t(gen()); b[0] &= 0x3f; b[31] |= 1; return SecretKey::from_bytes(b); };
    std::vector<Bytes> roots;
    for (int j = 0; j < 5; j++) roots.push_back(Bytes(30 + j, uint8_t(0xB0 + j)));
    const uint32_t named[3] = {0, 4, 2};                                              // the entries the sets name: the first, the last, one between
    MessageTable table(1);                                                            // grows with the appends
    CHECK(table.append(std::vector<Bytes>(roots.begin(), roots.begin() + 2)) == 0);
    CHECK(table.append(std::vector<Bytes>(roots.begin() + 2, roots.end())) == 2);
    CHECK(table.size() == 5);
    std::vector<SecretKey> sks; std::vector<AggregateSignature> sigs(9); std::vector<AggregatePublicKey> apks;
    for (int i = 0; i < 9; i++) {
        sks.push_back(rand_sk());
        sigs[i].add(Signature::new_(roots[named[i % 3]], sks[i]));
        apks.push_back(AggregatePublicKey::from_public_key(PublicKey::from_secret_key(sks[i])));
    }
    AggregateSignature wrong; wrong.add(Signature::new_(roots[named[4 % 3]], sks[5]));     // set 4 signed with set 5's key
    auto by_index = [&](bool bad) {
        std::vector<MessageTable::IndexedSet> v;
        for (int i = 0; i < 9; i++) v.emplace_back(bad && i == 4 ? &wrong : &sigs[i], &apks[i], named[i % 3]);
        return v;
    };
    auto spelled = [&](bool bad) {
        std::vector<Set> v;
        for (int i = 0; i < 9; i++) v.emplace_back(bad && i == 4 ? &wrong : &sigs[i], &apks[i], roots[named[i % 3]]);
        return v;
    };
    std::mt19937 g1(5), g2(5), g3(5);
    auto r1 = [&] { return uint8_t(g1()); };
    auto r2 = [&] { return uint8_t(g2()); };
    auto r3 = [&] { return uint8_t(g3()); };
    CHECK(table.verify_multiple_aggregate_signatures(r1, by_index(false)));
    CHECK(!table.verify_multiple_aggregate_signatures(r1, by_index(true)));
    auto good = table.verify_multiple_aggregate_signatures_locate(r2, by_index(false));
    CHECK(good.first && good.second == std::vector<bool>(9, true));
    auto got = table.verify_multiple_aggregate_signatures_locate(r2, by_index(true));
    std::vector<bool> want(9, true); want[4] = false;
    CHECK(!got.first && got.second == want);
    // the reference's method on the spelled-out messages, a generator with the same seed: same bools, same generator state afterwards
    CHECK(AggregateSignature::verify_multiple_aggregate_signatures(r3, spelled(false)));
    CHECK(!AggregateSignature::verify_multiple_aggregate_signatures(r3, spelled(true)));
    const auto a = g1(), b = g2(), c = g3();
    CHECK(a == b && b == c);
    // an index that names no entry is refused, an empty iterator accepts
    bool threw = false;
    try { auto v = by_index(false); std::get<2>(v[3]) = 5; (void)table.verify_multiple_aggregate_signatures(r1, v); } catch (const std::exception&) { threw = true; }
    CHECK(threw);
    { auto e = table.verify_multiple_aggregate_signatures_locate(r1, {}); CHECK(e.first && e.second.empty()); }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("all C++ verify_multiple message table checks passed\n");
    return 0;
}

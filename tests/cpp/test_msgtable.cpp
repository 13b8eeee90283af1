// MessageTable of include/milagro_bls.hpp (mbls_msgtable_*, mbls_fast_aggregate_verify_batch_msgtable, mbls_stream_create_msgtable / mbls_stream_submit_msgidx): six
// items over a table of three messages, one of them with an index that names another message than its signers saw -- directly and through a stream, the same bools
// as one fast_aggregate_verify per item. Exit code 0 = all passed.
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
    const std::vector<Bytes> msgs = {Bytes(32, 1), Bytes(7, 2), Bytes(64, 3)};      // messages of any length each
    const int n = 6;
    std::vector<uint32_t> idx = {2, 1, 0, 1, 2, 0};                                 // item 0 names entry 2, item 2 names entry 0
    std::vector<SecretKey> sks; std::vector<PublicKey> pks;
    for (int i = 0; i < 2 * n; i++) { sks.push_back(rand_sk()); pks.push_back(PublicKey::from_secret_key(sks.back())); }
    std::vector<AggregateSignature> sigs(n); std::vector<std::vector<const PublicKey*>> keys(n);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 2; j++) { sigs[i].add(Signature::new_(msgs[idx[i]], sks[2 * i + j])); keys[i].push_back(&pks[2 * i + j]); }
    {
        MessageTable table(2);                                                      // grows once
        CHECK(table.size() == 0);
        CHECK(table.append(msgs[0]) == 0);
        CHECK(table.append(std::vector<Bytes>{msgs[1], msgs[2]}) == 1);
        CHECK(table.size() == 3);
        auto good = fast_aggregate_verify_batch_msgtable(sigs, table, idx, keys);
        CHECK(good.size() == size_t(n));
        for (int i = 0; i < n; i++) CHECK(good[i] && sigs[i].fast_aggregate_verify(msgs[idx[i]], keys[i]));
        std::vector<uint32_t> wrong = idx; wrong[3] = 0;                            // signed over message 1, names entry 0
        auto got = fast_aggregate_verify_batch_msgtable(sigs, table, wrong, keys);
        for (int i = 0; i < n; i++) CHECK(got[i] == (i != 3));
        CHECK(!sigs[3].fast_aggregate_verify(msgs[0], keys[3]));
        {
            VerifyStream vs(table, MBLS_STREAM_FULL_ROUNDS, 64);
            auto t1 = vs.submit(sigs, idx, keys);
            auto t2 = vs.submit(sigs, wrong, keys);
            bool refused = false;                                                   // clear under a pending call
            try { table.clear(); } catch (const DeviceError&) { refused = true; } catch (const AmclError&) { refused = true; }
            CHECK(refused && table.size() == 3);
            bool mixed = false;                                                     // the message-carrying submit is not for this stream
            try { vs.submit(sigs, std::vector<Bytes>(n, msgs[0]), keys); } catch (const DeviceError&) { mixed = true; }
            CHECK(mixed);
            vs.flush();
            auto r1 = t1.get(), r2 = t2.get();
            for (int i = 0; i < n; i++) { CHECK(r1[i]); CHECK(r2[i] == (i != 3)); }
            CHECK(vs.stats().calls == 2);
        }
        wrong[3] = 3;                                                               // names no entry: refused before anything runs
        bool threw = false;
        try { fast_aggregate_verify_batch_msgtable(sigs, table, wrong, keys); } catch (const std::invalid_argument&) { threw = true; }
        CHECK(threw);
        CHECK(fast_aggregate_verify_batch_msgtable({}, table, {}, {}).empty());
        table.clear();
        CHECK(table.size() == 0 && table.append(msgs[2]) == 0);                     // index 0 names the new message
        std::vector<Signature> one = {Signature::new_(msgs[2], sks[0])};
        CHECK(verify_batch_msgtable(one, table, {0}, {&pks[0]})[0]);
        CHECK(!verify_batch_msgtable(one, table, {0}, {&pks[1]})[0]);
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("all C++ message table checks passed\n");
    return 0;
}

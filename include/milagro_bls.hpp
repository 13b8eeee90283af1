// milagro_bls.hpp -- C++ host-side mirror of the reference's public API (reference src/lib.rs:17-22) over the C ABI of
// libmbls_hip.so (include/mbls.h). Header-only; same type and method names, argument meaning and error behaviour as
// the Rust crate, so code written against milagro_bls reads the same:
//
//     reference (Rust)                                   here (C++17)
//     PublicKey::from_bytes(&[u8]) -> Result<..>         PublicKey::from_bytes(bytes)  (throws AmclError)
//     Signature::new(msg, &sk)                           Signature::new_(msg, sk)      ("new" is a keyword)
//     sig.verify(msg, &pk) -> bool                       sig.verify(msg, pk) -> bool
//     AggregateSignature::fast_aggregate_verify(..)      same
//     AggregateSignature::verify_multiple_aggregate_signatures(rng, iter)   same, rng = any callable returning uint8_t
//     (one call of it per batch, batch after batch)      AggregateSignature::verify_multiple_aggregate_signatures_batches(rng, batches) -> vector<bool>, ONE call
//     (the same over sets that share messages)            AggregateSignature::verify_multiple_aggregate_signatures_shared_msgs(rng, iter): one hash and, where it pays, one Miller loop per message
//     (... and which sets of a rejected call)             AggregateSignature::verify_multiple_aggregate_signatures_shared_msgs_locate(rng, iter): the bool and one bool per set
//     (... over a resident message table)                 MessageTable::verify_multiple_aggregate_signatures[_locate](rng, iter): messages by table index, nothing hashed
//
// Every curve / pairing operation runs in the HIP kernels; there is no CPU fallback: constructing the first object without a
// GPU throws DeviceError. The only host arithmetic is SecretKey::key_generate (HKDF-SHA-256 + one reduction mod r), which the
// reference also does on the host (src/keys.rs:45-77).
// Threads: all objects go through one process-wide mbls_ctx; every C ABI entry takes that context's lock, so the types can be used
// from any number of threads like the reference's -- calls are serialised on the one GPU.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <deque>
#include <exception>
#include <map>
#include <memory>
#include <mutex>
#include <random>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>
#include "mbls.h"

namespace milagro_bls {

constexpr size_t G1_BYTES = MBLS_G1_BYTES;                 // reference src/lib.rs:20
constexpr size_t G2_BYTES = MBLS_G2_BYTES;
constexpr size_t SECRET_KEY_BYTES = MBLS_SECRET_KEY_BYTES;
using Bytes = std::vector<uint8_t>;

// amcl::errors::AmclError (reference src/amcl_utils.rs:11): the variants the reference uses
struct AmclError : std::runtime_error {
    enum Kind { InvalidG1Size = 1, InvalidG2Size = 2, InvalidPoint = 3, AggregateEmptyPoints = 4, InvalidSecretKeySize = 5, InvalidSecretKeyRange = 6 };
    Kind kind;
    explicit AmclError(int k) : std::runtime_error("AmclError " + std::to_string(k)), kind(static_cast<Kind>(k)) {}
};
struct DeviceError : std::runtime_error { using std::runtime_error::runtime_error; };

namespace detail {
inline mbls_ctx* ctx() {
    static mbls_ctx* c = [] {
        mbls_ctx* p = nullptr;
        if (mbls_ctx_create(&p, 0) != MBLS_OK) throw DeviceError("mbls_ctx_create failed: no MI355X / HIP device (there is no CPU fallback)");
        return p;
    }();
    return c;
}
inline void check(int rc) {
    if (rc == MBLS_OK) return;
    if (rc >= MBLS_ERR_DEVICE) throw DeviceError(std::string("mbls device error: ") + mbls_last_error(ctx()));
    throw AmclError(rc);
}
}  // namespace detail

// ---- host-side SHA-256 / HMAC / HKDF for KeyGenerate (reference src/keys.rs:45-77 uses amcl's HASH256::hkdf_extract / hkdf_extend)
namespace detail {
struct Sha256 {
    uint32_t h[8]; uint8_t buf[64]; uint64_t len = 0; size_t fill = 0;
    Sha256() { static const uint32_t iv[8] = {0x6a09e667,0xbb67ae85,0x3c6ef372,0xa54ff53a,0x510e527f,0x9b05688c,0x1f83d9ab,0x5be0cd19}; std::memcpy(h, iv, 32); }
    static uint32_t ror(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
    void block(const uint8_t* p) {
        static const uint32_t K[64] = {
            0x428a2f98,0x71374491,0xb5c0fbcf,0xe9b5dba5,0x3956c25b,0x59f111f1,0x923f82a4,0xab1c5ed5,0xd807aa98,0x12835b01,0x243185be,0x550c7dc3,0x72be5d74,0x80deb1fe,0x9bdc06a7,0xc19bf174,
            0xe49b69c1,0xefbe4786,0x0fc19dc6,0x240ca1cc,0x2de92c6f,0x4a7484aa,0x5cb0a9dc,0x76f988da,0x983e5152,0xa831c66d,0xb00327c8,0xbf597fc7,0xc6e00bf3,0xd5a79147,0x06ca6351,0x14292967,
            0x27b70a85,0x2e1b2138,0x4d2c6dfc,0x53380d13,0x650a7354,0x766a0abb,0x81c2c92e,0x92722c85,0xa2bfe8a1,0xa81a664b,0xc24b8b70,0xc76c51a3,0xd192e819,0xd6990624,0xf40e3585,0x106aa070,
            0x19a4c116,0x1e376c08,0x2748774c,0x34b0bcb5,0x391c0cb3,0x4ed8aa4a,0x5b9cca4f,0x682e6ff3,0x748f82ee,0x78a5636f,0x84c87814,0x8cc70208,0x90befffa,0xa4506ceb,0xbef9a3f7,0xc67178f2};
        uint32_t w[64];
        for (int i = 0; i < 16; i++) w[i] = (uint32_t(p[4 * i]) << 24) | (uint32_t(p[4 * i + 1]) << 16) | (uint32_t(p[4 * i + 2]) << 8) | p[4 * i + 3];
        for (int i = 16; i < 64; i++) w[i] = w[i - 16] + (ror(w[i - 15], 7) ^ ror(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] + (ror(w[i - 2], 17) ^ ror(w[i - 2], 19) ^ (w[i - 2] >> 10));
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; i++) {
            uint32_t t1 = hh + (ror(e, 6) ^ ror(e, 11) ^ ror(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
            uint32_t t2 = (ror(a, 2) ^ ror(a, 13) ^ ror(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    void update(const uint8_t* p, size_t n) {
        len += n;
        while (n) { size_t t = std::min(n, size_t(64) - fill); std::memcpy(buf + fill, p, t); fill += t; p += t; n -= t; if (fill == 64) { block(buf); fill = 0; } }
    }
    std::array<uint8_t, 32> finish() {
        uint64_t bits = len * 8; uint8_t pad = 0x80; update(&pad, 1);
        uint8_t z = 0; while (fill != 56) update(&z, 1);
        uint8_t lb[8]; for (int i = 0; i < 8; i++) lb[i] = uint8_t(bits >> (56 - 8 * i)); update(lb, 8);
        std::array<uint8_t, 32> o; for (int i = 0; i < 8; i++) { o[4 * i] = uint8_t(h[i] >> 24); o[4 * i + 1] = uint8_t(h[i] >> 16); o[4 * i + 2] = uint8_t(h[i] >> 8); o[4 * i + 3] = uint8_t(h[i]); }
        return o;
    }
};
inline std::array<uint8_t, 32> sha256(const Bytes& m) { Sha256 s; s.update(m.data(), m.size()); return s.finish(); }
inline std::array<uint8_t, 32> hmac_sha256(const Bytes& key, const Bytes& msg) {
    Bytes k = key; if (k.size() > 64) { auto d = sha256(k); k.assign(d.begin(), d.end()); } k.resize(64, 0);
    Bytes i(64), o(64); for (int j = 0; j < 64; j++) { i[j] = k[j] ^ 0x36; o[j] = k[j] ^ 0x5c; }
    i.insert(i.end(), msg.begin(), msg.end()); auto inner = sha256(i);
    o.insert(o.end(), inner.begin(), inner.end()); return sha256(o);
}
// HKDF-SHA-256 (RFC 5869; amcl's HASH256::hkdf_extract / hkdf_extend, reference src/keys.rs:62-69). An empty salt is HashLen zero bytes.
inline std::array<uint8_t, 32> hkdf_extract(const Bytes& salt, const Bytes& ikm) { return hmac_sha256(salt.empty() ? Bytes(32, 0) : salt, ikm); }
inline Bytes hkdf_expand(const std::array<uint8_t, 32>& prk, const Bytes& info, size_t len) {
    Bytes okm, t; uint8_t ctr = 1;
    while (okm.size() < len) {
        Bytes m = t; m.insert(m.end(), info.begin(), info.end()); m.push_back(ctr++);
        auto d = hmac_sha256(Bytes(prk.begin(), prk.end()), m); t.assign(d.begin(), d.end());
        okm.insert(okm.end(), t.begin(), t.end());
    }
    okm.resize(len); return okm;
}
// OS2IP(48 bytes) mod r -> 32 bytes big-endian (bitwise long division on 32-bit limbs; host-only, once per key)
inline std::array<uint8_t, 32> mod_r(const uint8_t okm[48]) {
    static const uint32_t R[9] = {0x00000001, 0xffffffff, 0xfffe5bfe, 0x53bda402, 0x09a1d805, 0x3339d808, 0x299d7d48, 0x73eda753, 0};
    uint32_t a[9] = {0};
    for (int bit = 0; bit < 384; bit++) {
        for (int j = 8; j > 0; j--) a[j] = (a[j] << 1) | (a[j - 1] >> 31);
        a[0] = (a[0] << 1) | ((okm[bit >> 3] >> (7 - (bit & 7))) & 1u);
        bool ge = true; for (int j = 8; j >= 0; j--) { if (a[j] != R[j]) { ge = a[j] > R[j]; break; } }
        if (ge) { uint64_t br = 0; for (int j = 0; j < 9; j++) { uint64_t d = uint64_t(a[j]) - R[j] - br; a[j] = uint32_t(d); br = (d >> 63) & 1; } }
    }
    std::array<uint8_t, 32> o; for (int j = 0; j < 8; j++) { uint32_t v = a[7 - j]; o[4 * j] = uint8_t(v >> 24); o[4 * j + 1] = uint8_t(v >> 16); o[4 * j + 2] = uint8_t(v >> 8); o[4 * j + 3] = uint8_t(v); }
    return o;
}
}  // namespace detail

// reference src/keys.rs:28-113 (host-only object; the scalar goes to the GPU only for signing)
class SecretKey {
    std::array<uint8_t, 32> x_{};
public:
    // KeyGenerate, reference src/keys.rs:45-77: HKDF-SHA-256 with the salt-rehash loop (KEY_SALT :24, L = 48 :26)
    static SecretKey key_generate(const Bytes& ikm, const Bytes& key_info = {}) {
        if (ikm.size() < 32) throw AmclError(AmclError::InvalidSecretKeySize);
        const char* ks = "BLS-SIG-KEYGEN-SALT-";
        Bytes salt(ks, ks + 20);
        SecretKey s;
        bool zero = true;
        while (zero) {
            auto hs = detail::sha256(salt); salt.assign(hs.begin(), hs.end());                          // salt = H(salt)
            Bytes ikm0 = ikm; ikm0.push_back(0);
            auto prk = detail::hkdf_extract(salt, ikm0);                                                // PRK = HKDF-Extract(salt, IKM || 0)
            Bytes info = key_info; info.push_back(0); info.push_back(48);                               // key_info || I2OSP(L, 2)
            Bytes okm = detail::hkdf_expand(prk, info, 48);                                             // OKM = HKDF-Expand(PRK, info, L)
            s.x_ = detail::mod_r(okm.data());                                                           // SK = OS2IP(OKM) mod r
            for (uint8_t v : s.x_) if (v) zero = false;
        }
        return s;
    }
    // SecretKey::random (src/keys.rs:36-39): 32 bytes of IKM from the caller's byte source (rng() returns one random byte)
    template <typename Rng> static SecretKey random(Rng&& rng) { Bytes ikm(32); for (auto& b : ikm) b = uint8_t(rng()); return key_generate(ikm); }
    static SecretKey random() { std::random_device rd; return random([&] { return uint8_t(rd()); }); }
    static SecretKey from_bytes(const Bytes& b) {                          // src/keys.rs:80-82, error cases :285-297
        static const uint8_t R[32] = {0x73,0xed,0xa7,0x53,0x29,0x9d,0x7d,0x48,0x33,0x39,0xd8,0x08,0x09,0xa1,0xd8,0x05,0x53,0xbd,0xa4,0x02,0xff,0xfe,0x5b,0xfe,0xff,0xff,0xff,0xff,0x00,0x00,0x00,0x01};
        if (b.size() != 32) throw AmclError(AmclError::InvalidSecretKeySize);
        bool zero = true; for (uint8_t v : b) if (v) zero = false;
        if (zero || std::memcmp(b.data(), R, 32) >= 0) throw AmclError(AmclError::InvalidSecretKeyRange);
        SecretKey s; std::memcpy(s.x_.data(), b.data(), 32); return s;
    }
    Bytes as_bytes() const { return Bytes(x_.begin(), x_.end()); }
    bool operator==(const SecretKey& o) const { return x_ == o.x_; }
    ~SecretKey() { volatile uint8_t* p = x_.data(); for (int i = 0; i < 32; i++) p[i] = 0; }   // zeroize on drop, src/keys.rs:109-113
};

// reference src/keys.rs:116-187; `point` is the 96-byte uncompressed form
struct PublicKey {
    std::array<uint8_t, 96> point{};
    static PublicKey from_secret_key(const SecretKey& sk) { PublicKey p; Bytes b = sk.as_bytes(); detail::check(mbls_pk_from_secret_key(detail::ctx(), b.data(), b.size(), p.point.data())); return p; }
    static PublicKey from_bytes(const Bytes& b) { PublicKey p; detail::check(mbls_pk_from_bytes(detail::ctx(), b.data(), b.size(), p.point.data())); return p; }
    static PublicKey from_bytes_unchecked(const Bytes& b) { PublicKey p; detail::check(mbls_pk_from_bytes_unchecked(detail::ctx(), b.data(), b.size(), p.point.data())); return p; }
    static PublicKey from_uncompressed_bytes(const Bytes& b) { PublicKey p; detail::check(mbls_pk_from_uncompressed_bytes(detail::ctx(), b.data(), b.size(), p.point.data())); return p; }
    std::array<uint8_t, 48> as_bytes() const { std::array<uint8_t, 48> o{}; detail::check(mbls_pk_as_bytes(detail::ctx(), point.data(), o.data())); return o; }
    std::array<uint8_t, 96> as_uncompressed_bytes() const { return point; }
    bool key_validate() const { return mbls_pk_key_validate(detail::ctx(), point.data()) == 1; }
    bool operator==(const PublicKey& o) const { return point == o.point; }
};

struct Keypair {                                                             // reference src/keys.rs:189-204
    SecretKey sk; PublicKey pk;
    template <typename Rng> static Keypair random(Rng&& rng) { SecretKey s = SecretKey::random(rng); PublicKey p = PublicKey::from_secret_key(s); return Keypair{s, p}; }
    static Keypair random() { SecretKey s = SecretKey::random(); PublicKey p = PublicKey::from_secret_key(s); return Keypair{s, p}; }
};

// reference src/signature.rs:9-51; `point` is the 96-byte compressed form
struct Signature {
    std::array<uint8_t, 96> point{};
    static Signature new_(const Bytes& msg, const SecretKey& sk) {
        Signature s; Bytes k = sk.as_bytes(); detail::check(mbls_sign(detail::ctx(), msg.data(), msg.size(), k.data(), k.size(), s.point.data())); return s;
    }
    bool verify(const Bytes& msg, const PublicKey& pk) const { return mbls_verify(detail::ctx(), point.data(), msg.data(), msg.size(), pk.point.data()) == 1; }
    static Signature from_bytes(const Bytes& b) { Signature s; detail::check(mbls_sig_from_bytes(detail::ctx(), b.data(), b.size(), s.point.data())); return s; }
    std::array<uint8_t, 96> as_bytes() const { return point; }
    bool operator==(const Signature& o) const { return point == o.point; }
};

// reference src/aggregates.rs:17-78
struct AggregatePublicKey {
    std::array<uint8_t, 96> point{};
    static AggregatePublicKey aggregate(const std::vector<const PublicKey*>& keys) {
        if (keys.empty()) throw AmclError(AmclError::AggregateEmptyPoints);
        Bytes flat; for (auto* k : keys) flat.insert(flat.end(), k->point.begin(), k->point.end());
        AggregatePublicKey a; detail::check(mbls_aggregate_public_keys(detail::ctx(), flat.data(), keys.size(), a.point.data())); return a;
    }
    static AggregatePublicKey into_aggregate(const std::vector<PublicKey>& keys) {
        std::vector<const PublicKey*> p; for (auto& k : keys) p.push_back(&k); return aggregate(p);
    }
    static AggregatePublicKey from_public_key(const PublicKey& k) { AggregatePublicKey a; a.point = k.point; return a; }
    void add(const PublicKey& k) { detail::check(mbls_aggregate_public_key_add(detail::ctx(), point.data(), k.point.data(), point.data())); }
    void add_aggregate(const AggregatePublicKey& o) { detail::check(mbls_aggregate_public_key_add(detail::ctx(), point.data(), o.point.data(), point.data())); }
    bool operator==(const AggregatePublicKey& o) const { return point == o.point; }
};

// reference src/aggregates.rs:83-334
struct AggregateSignature {
    std::array<uint8_t, 96> point{};
    AggregateSignature() { point[0] = 0xC0; }                                // AggregateSignature::new(): the point at infinity
    static AggregateSignature aggregate(const std::vector<const Signature*>& sigs) {      // src/aggregates.rs:100-106: one batched launch
        AggregateSignature a; if (sigs.empty()) return a;
        Bytes flat; for (auto* s : sigs) flat.insert(flat.end(), s->point.begin(), s->point.end());
        uint8_t e = 0; detail::check(mbls_aggregate_signatures_batch(detail::ctx(), flat.data(), nullptr, 1, uint32_t(sigs.size()), a.point.data(), &e)); detail::check(e);
        return a;
    }
    static AggregateSignature from_signature(const Signature& s) { AggregateSignature a; a.point = s.point; return a; }
    void add(const Signature& s) { detail::check(mbls_aggregate_signature_add(detail::ctx(), point.data(), s.point.data(), point.data())); }
    void add_aggregate(const AggregateSignature& o) { detail::check(mbls_aggregate_signature_add(detail::ctx(), point.data(), o.point.data(), point.data())); }
    bool aggregate_verify(const std::vector<Bytes>& msgs, const std::vector<const PublicKey*>& pks) const {
        Bytes flat_m, flat_p; std::vector<size_t> lens;
        for (auto& m : msgs) { flat_m.insert(flat_m.end(), m.begin(), m.end()); lens.push_back(m.size()); }
        for (auto* k : pks) flat_p.insert(flat_p.end(), k->point.begin(), k->point.end());
        return mbls_aggregate_verify(detail::ctx(), point.data(), flat_m.data(), lens.data(), msgs.size(), flat_p.data(), pks.size()) == 1;
    }
    bool fast_aggregate_verify(const Bytes& msg, const std::vector<const PublicKey*>& pks) const {
        Bytes flat; for (auto* k : pks) flat.insert(flat.end(), k->point.begin(), k->point.end());
        return mbls_fast_aggregate_verify(detail::ctx(), point.data(), msg.data(), msg.size(), flat.data(), pks.size()) == 1;
    }
    bool fast_aggregate_verify_pre_aggregated(const Bytes& msg, const AggregatePublicKey& apk) const {
        return mbls_fast_aggregate_verify_pre_aggregated(detail::ctx(), point.data(), msg.data(), msg.size(), apk.point.data()) == 1;
    }
    // one scalar as at reference src/aggregates.rs:280-287: 8 random bytes, big-endian i64, absolute value (as the release build wraps it), again on zero
    template <typename Rng> static uint64_t draw_scalar(Rng& rng) {
        uint64_t r = 0;
        while (r == 0) { uint64_t v = 0; for (int j = 0; j < 8; j++) v = (v << 8) | uint8_t(rng()); r = (v >> 63) ? (uint64_t(0) - v) : v; }
        return r;
    }
    // One call (mbls_verify_multiple_aggregate_signatures_rng): the library tests the signatures first and asks for the scalars of the sets in front of the first
    // bad one only -- the reference's order (its loop tests set i's signature for the subgroup, :272-275, BEFORE it draws rand[i] and returns at the first signature
    // outside G2: a rejected batch leaves the caller's generator where the reference would) without a second subgroup test. rng(): one random byte per call.
    template <typename Rng>
    static bool verify_multiple_aggregate_signatures(Rng&& rng, const std::vector<std::tuple<const AggregateSignature*, const AggregatePublicKey*, Bytes>>& sets) {
        if (sets.empty()) return mbls_verify_multiple_aggregate_signatures(detail::ctx(), nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0) == 1;
        Bytes sigs, apks, msgs; std::vector<uint64_t> moff{0};
        for (auto& s : sets) {
            sigs.insert(sigs.end(), std::get<0>(s)->point.begin(), std::get<0>(s)->point.end());
            apks.insert(apks.end(), std::get<1>(s)->point.begin(), std::get<1>(s)->point.end());
            msgs.insert(msgs.end(), std::get<2>(s).begin(), std::get<2>(s).end());
            moff.push_back(msgs.size());
        }
        using R = typename std::remove_reference<Rng>::type;
        struct src { R* rng; std::exception_ptr err; } u{&rng, nullptr};
        mbls_scalar_source draw = [](void* user, uint64_t* out, uint64_t count) {
            src* p = static_cast<src*>(user);
            try { for (uint64_t i = 0; i < count; i++) out[i] = draw_scalar(*p->rng); }
            catch (...) { p->err = std::current_exception(); for (uint64_t i = 0; i < count; i++) out[i] = 0; }        // never unwind through the C frames
        };
        const bool ok = mbls_verify_multiple_aggregate_signatures_rng(detail::ctx(), sigs.data(), apks.data(), msgs.data(), 0, moff.data(), sets.size(), draw, &u) == 1;
        if (u.err) std::rethrow_exception(u.err);
        return ok;
    }
    // Not in the reference: verify_multiple_aggregate_signatures(rng, sets) -- same sets, same bool, rng left in the same state -- for batches whose sets share
    // messages (mbls_verify_multiple_shared_msgs_rng): the messages are deduplicated here by their bytes, each distinct message is hashed once and, where it
    // pays, the check walks one Miller loop per message instead of one per set.
    template <typename Rng>
    static bool verify_multiple_aggregate_signatures_shared_msgs(Rng&& rng, const std::vector<std::tuple<const AggregateSignature*, const AggregatePublicKey*, Bytes>>& sets) {
        return vm_shared(rng, sets, nullptr);
    }
    // The same, and in the same call (mbls_verify_multiple_shared_msgs_locate_rng) WHICH sets of a rejected call are the bad ones: .first as above, .second one bool
    // per set. Every set of an accepted call reads true (a passing batch is not examined set by set); a set of a rejected call reads what the one-set call with
    // its scalar returns; a set at or behind the first signature outside G2 has no scalar (the reference never draws one) and reads false. rng is left where
    // verify_multiple_aggregate_signatures_shared_msgs leaves it.
    template <typename Rng>
    static std::pair<bool, std::vector<bool>> verify_multiple_aggregate_signatures_shared_msgs_locate(
            Rng&& rng, const std::vector<std::tuple<const AggregateSignature*, const AggregatePublicKey*, Bytes>>& sets) {
        std::vector<bool> per_set;
        const bool ok = vm_shared(rng, sets, &per_set);
        return {ok, per_set};
    }
private:
    template <typename Rng>
    static bool vm_shared(Rng& rng, const std::vector<std::tuple<const AggregateSignature*, const AggregatePublicKey*, Bytes>>& sets, std::vector<bool>* per_set) {
        if (sets.empty()) return true;
        Bytes sigs, apks, msgs; std::vector<uint64_t> moff{0}; std::vector<uint32_t> idx; std::map<Bytes, uint32_t> index;
        for (auto& s : sets) {
            sigs.insert(sigs.end(), std::get<0>(s)->point.begin(), std::get<0>(s)->point.end());
            apks.insert(apks.end(), std::get<1>(s)->point.begin(), std::get<1>(s)->point.end());
            auto it = index.find(std::get<2>(s));
            if (it == index.end()) {
                it = index.emplace(std::get<2>(s), uint32_t(index.size())).first;
                msgs.insert(msgs.end(), std::get<2>(s).begin(), std::get<2>(s).end());
                moff.push_back(msgs.size());
            }
            idx.push_back(it->second);
        }
        using R = typename std::remove_reference<Rng>::type;
        struct src { R* rng; std::exception_ptr err; } u{&rng, nullptr};
        mbls_scalar_source draw = [](void* user, uint64_t* out, uint64_t count) {
            src* p = static_cast<src*>(user);
            try { for (uint64_t i = 0; i < count; i++) out[i] = draw_scalar(*p->rng); }
            catch (...) { p->err = std::current_exception(); for (uint64_t i = 0; i < count; i++) out[i] = 0; }        // never unwind through the C frames
        };
        uint8_t ok = 0;
        std::vector<uint8_t> sres(per_set ? sets.size() : 0);
        const int rc = per_set
            ? mbls_verify_multiple_shared_msgs_locate_rng(detail::ctx(), sigs.data(), apks.data(), msgs.data(), 0, moff.data(), index.size(), idx.data(), sets.size(), &ok,
                                                          sres.data(), nullptr, draw, &u)
            : mbls_verify_multiple_shared_msgs_rng(detail::ctx(), sigs.data(), apks.data(), msgs.data(), 0, moff.data(), index.size(), idx.data(), sets.size(), &ok, draw, &u);
        if (u.err) std::rethrow_exception(u.err);
        detail::check(rc);
        if (per_set) per_set->assign(sres.begin(), sres.end());
        return ok == 1;
    }
public:
    // Not in the reference: what verify_multiple_aggregate_signatures(rng, batch) returns for every batch of `batches`, called once per batch in order -- as ONE
    // call (mbls_verify_multiple_batches_rng), for about the cost of one such call. One bool per batch; a bad batch rejects itself and nothing else. The scalars
    // are drawn in the order those calls would draw them (for every batch, the sets in front of its first signature outside G2): rng is left where they leave it.
    template <typename Rng>
    static std::vector<bool> verify_multiple_aggregate_signatures_batches(
            Rng&& rng, const std::vector<std::vector<std::tuple<const AggregateSignature*, const AggregatePublicKey*, Bytes>>>& batches) {
        std::vector<bool> out;
        if (batches.empty()) return out;
        Bytes sigs, apks, msgs; std::vector<uint64_t> moff{0}; std::vector<uint32_t> boff{0};
        for (auto& b : batches) {
            for (auto& s : b) {
                sigs.insert(sigs.end(), std::get<0>(s)->point.begin(), std::get<0>(s)->point.end());
                apks.insert(apks.end(), std::get<1>(s)->point.begin(), std::get<1>(s)->point.end());
                msgs.insert(msgs.end(), std::get<2>(s).begin(), std::get<2>(s).end());
                moff.push_back(msgs.size());
            }
            boff.push_back(uint32_t(moff.size() - 1));
        }
        using R = typename std::remove_reference<Rng>::type;
        struct src { R* rng; std::exception_ptr err; } u{&rng, nullptr};
        mbls_scalar_source draw = [](void* user, uint64_t* o, uint64_t count) {
            src* p = static_cast<src*>(user);
            try { for (uint64_t i = 0; i < count; i++) o[i] = draw_scalar(*p->rng); }
            catch (...) { p->err = std::current_exception(); for (uint64_t i = 0; i < count; i++) o[i] = 0; }        // never unwind through the C frames
        };
        Bytes res(batches.size(), 0);
        const int rc = mbls_verify_multiple_batches_rng(detail::ctx(), sigs.data(), apks.data(), msgs.data(), 0, moff.data(), moff.size() - 1, boff.data(), 0,
                                                        batches.size(), res.data(), draw, &u);
        if (u.err) std::rethrow_exception(u.err);
        detail::check(rc);
        for (uint8_t r : res) out.push_back(r == 1);
        return out;
    }
    // The same, and in the same call (mbls_verify_multiple_batches_locate_rng) WHICH sets of the rejected batches are the bad ones: .first as above, .second one bool
    // per set of every batch. Every set of an accepted batch reads true -- a passing batch is not examined set by set: the batch check is the statement
    // verify_multiple makes. A set of a rejected batch reads what the one-set batch with its scalar returns; a set at or behind the batch's first signature outside
    // G2 has no scalar (the reference never draws one) and reads false. rng is left where verify_multiple_aggregate_signatures_batches leaves it.
    template <typename Rng>
    static std::pair<std::vector<bool>, std::vector<std::vector<bool>>> verify_multiple_aggregate_signatures_batches_locate(
            Rng&& rng, const std::vector<std::vector<std::tuple<const AggregateSignature*, const AggregatePublicKey*, Bytes>>>& batches) {
        std::pair<std::vector<bool>, std::vector<std::vector<bool>>> out;
        if (batches.empty()) return out;
        Bytes sigs, apks, msgs; std::vector<uint64_t> moff{0}; std::vector<uint32_t> boff{0};
        for (auto& b : batches) {
            for (auto& s : b) {
                sigs.insert(sigs.end(), std::get<0>(s)->point.begin(), std::get<0>(s)->point.end());
                apks.insert(apks.end(), std::get<1>(s)->point.begin(), std::get<1>(s)->point.end());
                msgs.insert(msgs.end(), std::get<2>(s).begin(), std::get<2>(s).end());
                moff.push_back(msgs.size());
            }
            boff.push_back(uint32_t(moff.size() - 1));
        }
        using R = typename std::remove_reference<Rng>::type;
        struct src { R* rng; std::exception_ptr err; } u{&rng, nullptr};
        mbls_scalar_source draw = [](void* user, uint64_t* o, uint64_t count) {
            src* p = static_cast<src*>(user);
            try { for (uint64_t i = 0; i < count; i++) o[i] = draw_scalar(*p->rng); }
            catch (...) { p->err = std::current_exception(); for (uint64_t i = 0; i < count; i++) o[i] = 0; }        // never unwind through the C frames
        };
        const size_t n = moff.size() - 1;
        Bytes res(batches.size(), 0), sres(n ? n : 1, 0);
        const int rc = mbls_verify_multiple_batches_locate_rng(detail::ctx(), sigs.data(), apks.data(), msgs.data(), 0, moff.data(), n, boff.data(), 0,
                                                               batches.size(), res.data(), sres.data(), nullptr, draw, &u);
        if (u.err) std::rethrow_exception(u.err);
        detail::check(rc);
        for (size_t b = 0; b < batches.size(); b++) {
            out.first.push_back(res[b] == 1);
            std::vector<bool> per;
            for (uint32_t i = boff[b]; i < boff[b + 1]; i++) per.push_back(sres[i] == 1);
            out.second.push_back(per);
        }
        return out;
    }
    // the same check with the sets cut into one shard per device of a multi-device handle (mbls_multi_create): same bool, same RNG order, ONE call
    // (mbls_multi_verify_multiple_aggregate_signatures_rng: every device tests its shard's signatures first, the scalars are asked for once)
    template <typename Rng>
    static bool verify_multiple_aggregate_signatures(mbls_multi* devices, Rng&& rng, const std::vector<std::tuple<const AggregateSignature*, const AggregatePublicKey*, Bytes>>& sets) {
        if (sets.empty()) return true;
        Bytes sigs, apks, msgs; std::vector<uint64_t> moff{0};
        for (auto& s : sets) {
            sigs.insert(sigs.end(), std::get<0>(s)->point.begin(), std::get<0>(s)->point.end());
            apks.insert(apks.end(), std::get<1>(s)->point.begin(), std::get<1>(s)->point.end());
            msgs.insert(msgs.end(), std::get<2>(s).begin(), std::get<2>(s).end());
            moff.push_back(msgs.size());
        }
        using R = typename std::remove_reference<Rng>::type;
        struct src { R* rng; std::exception_ptr err; } u{&rng, nullptr};
        mbls_scalar_source draw = [](void* user, uint64_t* out, uint64_t count) {
            src* p = static_cast<src*>(user);
            try { for (uint64_t i = 0; i < count; i++) out[i] = draw_scalar(*p->rng); }
            catch (...) { p->err = std::current_exception(); for (uint64_t i = 0; i < count; i++) out[i] = 0; }
        };
        const bool ok = mbls_multi_verify_multiple_aggregate_signatures_rng(devices, sigs.data(), apks.data(), msgs.data(), 0, moff.data(), sets.size(), draw, &u) == 1;
        if (u.err) std::rethrow_exception(u.err);
        return ok;
    }
    static AggregateSignature from_bytes(const Bytes& b) { AggregateSignature a; detail::check(mbls_sig_from_bytes(detail::ctx(), b.data(), b.size(), a.point.data())); return a; }
    std::array<uint8_t, 96> as_bytes() const { return point; }
    bool operator==(const AggregateSignature& o) const { return point == o.point; }
};

// Several GPUs behind one handle (mbls_multi_*; not part of the reference's API): contiguous shards, one context and one host thread per
// device inside the library, results written in place. Items are independent (reference src/aggregates.rs:177-215 keeps no state).
// n x AggregateSignature::aggregate_verify (src/aggregates.rs:130-170) in one launch chain: item i = (sigs[i], its messages, its keys); an item
// with a different number of messages and keys, or with none, is false like the reference's early return (:131-133)
inline std::vector<bool> aggregate_verify_batch(const std::vector<AggregateSignature>& sigs, const std::vector<std::vector<Bytes>>& msgs,
                                                const std::vector<std::vector<const PublicKey*>>& keys) {
    const size_t n = sigs.size();
    if (msgs.size() != n || keys.size() != n) throw std::invalid_argument("one message list and one key list per signature");
    Bytes s, m, p; std::vector<uint64_t> moff{0}; std::vector<uint32_t> poff{0}; std::vector<bool> mismatch(n, false);
    for (size_t i = 0; i < n; i++) {
        s.insert(s.end(), sigs[i].point.begin(), sigs[i].point.end());
        if (msgs[i].size() != keys[i].size()) mismatch[i] = true;          // enters the batch without pairs: false
        else for (size_t j = 0; j < keys[i].size(); j++) {
            m.insert(m.end(), msgs[i][j].begin(), msgs[i][j].end()); moff.push_back(m.size());
            p.insert(p.end(), keys[i][j]->point.begin(), keys[i][j]->point.end());
        }
        if (p.size() / 96 > 0xFFFFFFFFull) throw std::invalid_argument("aggregate_verify_batch: pair indices are 32-bit");
        poff.push_back(uint32_t(p.size() / 96));
    }
    std::vector<uint8_t> res(n ? n : 1);
    detail::check(mbls_aggregate_verify_batch(detail::ctx(), s.data(), m.data(), 0, moff.data(), p.data(), poff.data(), 0, n, res.data(), nullptr));
    std::vector<bool> out(n);
    for (size_t i = 0; i < n; i++) out[i] = res[i] == 1 && !mismatch[i];
    return out;
}

// n x AggregateSignature::fast_aggregate_verify (src/aggregates.rs:177-215) over a LIST of messages (mbls_fast_aggregate_verify_batch_shared_msgs; not part of the
// reference's API, whose hash_to_curve sits inside every verify): item i = (sigs[i], msgs[msg_idx[i]], keys[i]). The members of a committee sign the same message:
// every listed message is hashed to G2 once, whatever the number of items that name it. The same bools as one fast_aggregate_verify per item.
inline std::vector<bool> fast_aggregate_verify_batch_shared_msgs(const std::vector<AggregateSignature>& sigs, const std::vector<Bytes>& msgs,
                                                                 const std::vector<uint32_t>& msg_idx, const std::vector<std::vector<const PublicKey*>>& keys) {
    const size_t n = sigs.size();
    if (msg_idx.size() != n || keys.size() != n) throw std::invalid_argument("one message index and one key list per signature");
    if (msgs.size() > 0xFFFFFFFFull) throw std::invalid_argument("fast_aggregate_verify_batch_shared_msgs: message indices are 32-bit");
    for (uint32_t j : msg_idx) if (j >= msgs.size()) throw std::invalid_argument("fast_aggregate_verify_batch_shared_msgs: an index names no message of the list");
    Bytes s, m, p; std::vector<uint64_t> moff{0}; std::vector<uint32_t> koff{0};
    for (auto& x : msgs) { m.insert(m.end(), x.begin(), x.end()); moff.push_back(m.size()); }
    for (size_t i = 0; i < n; i++) {
        s.insert(s.end(), sigs[i].point.begin(), sigs[i].point.end());
        for (auto* k : keys[i]) p.insert(p.end(), k->point.begin(), k->point.end());
        if (p.size() / 96 > 0xFFFFFFFFull) throw std::invalid_argument("fast_aggregate_verify_batch_shared_msgs: key indices are 32-bit");
        koff.push_back(uint32_t(p.size() / 96));
    }
    std::vector<uint8_t> res(n ? n : 1);
    detail::check(mbls_fast_aggregate_verify_batch_shared_msgs(detail::ctx(), s.data(), m.data(), 0, moff.data(), msgs.size(), msg_idx.data(), p.data(), MBLS_PK_UNCOMPRESSED,
                                                               koff.data(), n, 0, res.data(), nullptr));
    std::vector<bool> out(n);
    for (size_t i = 0; i < n; i++) out[i] = res[i] == 1;
    return out;
}

// A resident message table on the library's context (include/mbls.h, "resident message table"; not part of the reference's API): every appended message is hashed
// to G2 once and stays in device memory; verifications -- direct ones below, or calls of a VerifyStream made over the table -- name their messages by index, in
// any later call. Indices start at 0 and never change until clear(). Destroy the table after the streams made over it.
class MessageTable {
    mbls_msgtable* h_ = nullptr;
public:
    explicit MessageTable(uint64_t capacity_hint = 0) { detail::check(mbls_msgtable_create(detail::ctx(), capacity_hint, &h_)); }
    MessageTable(const MessageTable&) = delete; MessageTable& operator=(const MessageTable&) = delete;
    ~MessageTable() { mbls_msgtable_destroy(h_); }
    mbls_msgtable* handle() const { return h_; }
    uint64_t size() const { return mbls_msgtable_size(h_); }
    // messages of any length each -> the index of the first; message j is entry first + j
    uint64_t append(const std::vector<Bytes>& msgs) {
        Bytes m; std::vector<uint64_t> moff{0};
        for (auto& x : msgs) { m.insert(m.end(), x.begin(), x.end()); moff.push_back(m.size()); }
        uint64_t first = 0;
        detail::check(mbls_msgtable_append(h_, m.data(), 0, moff.data(), msgs.size(), &first));
        return first;
    }
    uint64_t append(const Bytes& msg) { return append(std::vector<Bytes>{msg}); }
    // the compressed point of entry i: what hash_to_curve gives for its message
    std::array<uint8_t, 96> get(uint64_t i) const {
        std::array<uint8_t, 96> o{}; uint8_t e = 0;
        detail::check(mbls_msgtable_get(h_, i, 1, o.data(), &e)); detail::check(e);
        return o;
    }
    // size back to 0, capacity kept; refused (DeviceError) while a stream made over the table has calls that have not completed
    void clear() { detail::check(mbls_msgtable_clear(h_)); }
    // AggregateSignature::verify_multiple_aggregate_signatures over sets (signature, aggregate key, entry index) whose messages are entries of this table
    // (mbls_verify_multiple_msgtable_rng): the same bool as that method on the spelled-out messages, rng left in the same state, nothing hashed in the call.
    // An index that names no entry throws (DeviceError). rng(): one random byte per call.
    typedef std::tuple<const AggregateSignature*, const AggregatePublicKey*, uint32_t> IndexedSet;
    template <typename Rng>
    bool verify_multiple_aggregate_signatures(Rng&& rng, const std::vector<IndexedSet>& sets) const { return vm(rng, sets, nullptr); }
    // The same, and in the same call (mbls_verify_multiple_msgtable_locate_rng) which sets of a rejected call are the bad ones, with the semantics of
    // AggregateSignature::verify_multiple_aggregate_signatures_shared_msgs_locate.
    template <typename Rng>
    std::pair<bool, std::vector<bool>> verify_multiple_aggregate_signatures_locate(Rng&& rng, const std::vector<IndexedSet>& sets) const {
        std::vector<bool> per_set;
        const bool ok = vm(rng, sets, &per_set);
        return {ok, per_set};
    }
private:
    template <typename Rng>
    bool vm(Rng& rng, const std::vector<IndexedSet>& sets, std::vector<bool>* per_set) const {
        if (sets.empty()) return true;
        Bytes sigs, apks; std::vector<uint32_t> idx;
        for (auto& s : sets) {
            sigs.insert(sigs.end(), std::get<0>(s)->point.begin(), std::get<0>(s)->point.end());
            apks.insert(apks.end(), std::get<1>(s)->point.begin(), std::get<1>(s)->point.end());
            idx.push_back(std::get<2>(s));
        }
        using R = typename std::remove_reference<Rng>::type;
        struct src { R* rng; std::exception_ptr err; } u{&rng, nullptr};
        mbls_scalar_source draw = [](void* user, uint64_t* out, uint64_t count) {
            src* p = static_cast<src*>(user);
            try { for (uint64_t i = 0; i < count; i++) out[i] = AggregateSignature::draw_scalar(*p->rng); }
            catch (...) { p->err = std::current_exception(); for (uint64_t i = 0; i < count; i++) out[i] = 0; }        // never unwind through the C frames
        };
        uint8_t ok = 0;
        std::vector<uint8_t> sres(per_set ? sets.size() : 0);
        const int rc = per_set
            ? mbls_verify_multiple_msgtable_locate_rng(detail::ctx(), sigs.data(), apks.data(), h_, idx.data(), sets.size(), &ok, sres.data(), nullptr, draw, &u)
            : mbls_verify_multiple_msgtable_rng(detail::ctx(), sigs.data(), apks.data(), h_, idx.data(), sets.size(), &ok, draw, &u);
        if (u.err) std::rethrow_exception(u.err);
        detail::check(rc);
        if (per_set) per_set->assign(sres.begin(), sres.end());
        return ok == 1;
    }
};
namespace detail {
inline void flatten_items(const char* what, const std::vector<AggregateSignature>& sigs, const MessageTable& table, const std::vector<uint32_t>& msg_idx,
                          const std::vector<std::vector<const PublicKey*>>& keys, Bytes& s, Bytes& p, std::vector<uint32_t>& koff) {
    const size_t n = sigs.size();
    if (msg_idx.size() != n || keys.size() != n) throw std::invalid_argument(std::string(what) + ": one message index and one key list per signature");
    const uint64_t size = table.size();
    for (uint32_t j : msg_idx) if (j >= size) throw std::invalid_argument(std::string(what) + ": an index names no entry of the message table");
    koff.assign(1, 0);
    for (size_t i = 0; i < n; i++) {
        s.insert(s.end(), sigs[i].point.begin(), sigs[i].point.end());
        for (auto* k : keys[i]) p.insert(p.end(), k->point.begin(), k->point.end());
        if (p.size() / 96 > 0xFFFFFFFFull) throw std::invalid_argument(std::string(what) + ": key indices are 32-bit");
        koff.push_back(uint32_t(p.size() / 96));
    }
}
}  // namespace detail
// n x AggregateSignature::fast_aggregate_verify over a resident message table (mbls_fast_aggregate_verify_batch_msgtable): item i = (sigs[i], entry msg_idx[i],
// keys[i]); nothing is hashed. The same bools as one fast_aggregate_verify per item with the entry's message.
inline std::vector<bool> fast_aggregate_verify_batch_msgtable(const std::vector<AggregateSignature>& sigs, const MessageTable& table, const std::vector<uint32_t>& msg_idx,
                                                              const std::vector<std::vector<const PublicKey*>>& keys) {
    Bytes s, p; std::vector<uint32_t> koff;
    detail::flatten_items("fast_aggregate_verify_batch_msgtable", sigs, table, msg_idx, keys, s, p, koff);
    const size_t n = sigs.size();
    std::vector<uint8_t> res(n ? n : 1);
    detail::check(mbls_fast_aggregate_verify_batch_msgtable(detail::ctx(), s.data(), table.handle(), msg_idx.data(), p.data(), MBLS_PK_UNCOMPRESSED, koff.data(), n, 0,
                                                            res.data(), nullptr));
    std::vector<bool> out(n);
    for (size_t i = 0; i < n; i++) out[i] = res[i] == 1;
    return out;
}
// n x Signature::verify over a resident message table (mbls_verify_batch_msgtable): item i = (sigs[i], entry msg_idx[i], keys[i])
inline std::vector<bool> verify_batch_msgtable(const std::vector<Signature>& sigs, const MessageTable& table, const std::vector<uint32_t>& msg_idx,
                                               const std::vector<const PublicKey*>& keys) {
    const size_t n = sigs.size();
    if (msg_idx.size() != n || keys.size() != n) throw std::invalid_argument("verify_batch_msgtable: one message index and one key per signature");
    const uint64_t size = table.size();
    for (uint32_t j : msg_idx) if (j >= size) throw std::invalid_argument("verify_batch_msgtable: an index names no entry of the message table");
    Bytes s, p;
    for (size_t i = 0; i < n; i++) { s.insert(s.end(), sigs[i].point.begin(), sigs[i].point.end()); p.insert(p.end(), keys[i]->point.begin(), keys[i]->point.end()); }
    std::vector<uint8_t> res(n ? n : 1);
    detail::check(mbls_verify_batch_msgtable(detail::ctx(), s.data(), table.handle(), msg_idx.data(), p.data(), MBLS_PK_UNCOMPRESSED, n, res.data(), nullptr));
    std::vector<bool> out(n);
    for (size_t i = 0; i < n; i++) out[i] = res[i] == 1;
    return out;
}
// the same as fast_aggregate_verify_batch_msgtable with the keys named by index into a resident key table of the library's context
// (mbls_fast_aggregate_verify_batch_indexed_msgtable): item i uses key-table entries key_idx[i]
inline std::vector<bool> fast_aggregate_verify_batch_indexed_msgtable(const mbls_keytable* key_table, const std::vector<AggregateSignature>& sigs, const MessageTable& table,
                                                                      const std::vector<uint32_t>& msg_idx, const std::vector<std::vector<uint32_t>>& key_idx) {
    const size_t n = sigs.size();
    if (msg_idx.size() != n || key_idx.size() != n) throw std::invalid_argument("fast_aggregate_verify_batch_indexed_msgtable: one message index and one key index list per signature");
    const uint64_t size = table.size();
    for (uint32_t j : msg_idx) if (j >= size) throw std::invalid_argument("fast_aggregate_verify_batch_indexed_msgtable: an index names no entry of the message table");
    Bytes s; std::vector<uint32_t> flat, koff{0};
    for (size_t i = 0; i < n; i++) {
        s.insert(s.end(), sigs[i].point.begin(), sigs[i].point.end());
        flat.insert(flat.end(), key_idx[i].begin(), key_idx[i].end());
        if (flat.size() > 0xFFFFFFFFull) throw std::invalid_argument("fast_aggregate_verify_batch_indexed_msgtable: key offsets are 32-bit");
        koff.push_back(uint32_t(flat.size()));
    }
    std::vector<uint8_t> res(n ? n : 1);
    detail::check(mbls_fast_aggregate_verify_batch_indexed_msgtable(detail::ctx(), key_table, s.data(), table.handle(), msg_idx.data(), flat.data(), koff.data(), n, 0,
                                                                    res.data(), nullptr));
    std::vector<bool> out(n);
    for (size_t i = 0; i < n; i++) out[i] = res[i] == 1;
    return out;
}

// Committee table (mbls_committees_*): ordered member lists over a resident key table of the library's context, each with its cached key sum; a verification names a
// committee and carries the participation bits as serialized by SSZ (bit j = member j; bits at or above the committee's size are ignored). Destroy it before the key
// table it was made over.
class CommitteeTable {
    mbls_committees* h_ = nullptr;
public:
    explicit CommitteeTable(mbls_keytable* key_table, uint64_t capacity_hint = 0) { detail::check(mbls_committees_create(detail::ctx(), key_table, capacity_hint, &h_)); }
    CommitteeTable(const CommitteeTable&) = delete; CommitteeTable& operator=(const CommitteeTable&) = delete;
    ~CommitteeTable() { mbls_committees_destroy(h_); }
    mbls_committees* handle() const { return h_; }
    uint64_t count() const { return mbls_committees_count(h_); }
    uint32_t max_members() const { return mbls_committees_max_members(h_); }
    // one committee per member list (key-table indices, in member order) -> the id of the first
    uint64_t append(const std::vector<std::vector<uint32_t>>& committees) {
        std::vector<uint32_t> flat, off{0};
        for (const auto& c : committees) {
            flat.insert(flat.end(), c.begin(), c.end());
            if (flat.size() > 0xFFFFFFFFull) throw std::invalid_argument("CommitteeTable::append: member offsets are 32-bit");
            off.push_back(uint32_t(flat.size()));
        }
        if (flat.empty()) flat.push_back(0);
        uint64_t first = 0;
        detail::check(mbls_committees_append(h_, flat.data(), off.data(), committees.size(), &first));
        return first;
    }
    // the committee's full key sum (AggregatePublicKey::aggregate over its members), as cached on the device
    AggregatePublicKey aggregate_pubkey(uint64_t id, uint32_t* n_members = nullptr, bool* eligible = nullptr) const {
        AggregatePublicKey a; uint32_t m = 0, e = 0;
        detail::check(mbls_committees_get(h_, id, a.point.data(), &m, &e));
        if (n_members) *n_members = m;
        if (eligible) *eligible = e != 0;
        return a;
    }
    void clear() { detail::check(mbls_committees_clear(h_)); }
    // AggregateSignature::fast_aggregate_verify over attestations that span several committees (mbls_fast_aggregate_verify_batch_committee_span_msgtable): an
    // Electra attestation names the committees of its committee_bits, in order, and carries aggregation_bits -- the concatenation of their participation bits, as
    // serialized by SSZ (a Bitlist's delimiter may stay) -- under one signature over one entry of `table`. One bool per item: what fast_aggregate_verify gives on
    // the selected members spelled out. More than MBLS_SPAN_MAX_COMMITTEES ids, an id that names no committee, a field shorter than the committees' members or an
    // entry index that names nothing throws (DeviceError). status, when given, receives the items' MBLS_ST_* words.
    struct SpanItem { const AggregateSignature* signature; std::vector<uint32_t> committee_ids; Bytes aggregation_bits; uint32_t msg_index; };
    std::vector<bool> fast_aggregate_verify_spans(const std::vector<SpanItem>& items, const MessageTable& table, std::vector<uint32_t>* status = nullptr) const {
        const size_t n = items.size();
        if (status) status->assign(n, 0);
        if (!n) return {};
        size_t widest = 1;
        for (const auto& it : items) widest = std::max(widest, it.aggregation_bits.size());
        const uint32_t stride = uint32_t((widest + 3) / 4 * 4);                         // one stride for every field, a multiple of 4
        Bytes sigs, flat(size_t(stride) * n, 0); std::vector<uint32_t> ids, off{0}, idx, st(n, 0);
        for (size_t i = 0; i < n; i++) {
            const SpanItem& it = items[i];
            sigs.insert(sigs.end(), it.signature->point.begin(), it.signature->point.end());
            std::copy(it.aggregation_bits.begin(), it.aggregation_bits.end(), flat.begin() + size_t(stride) * i);
            ids.insert(ids.end(), it.committee_ids.begin(), it.committee_ids.end());
            if (ids.size() > 0xFFFFFFFFull) throw std::invalid_argument("fast_aggregate_verify_spans: span offsets are 32-bit");
            off.push_back(uint32_t(ids.size())); idx.push_back(it.msg_index);
        }
        const uint64_t n_ids = ids.size();
        if (ids.empty()) ids.push_back(0);
        std::vector<uint8_t> res(n, 0);
        detail::check(mbls_fast_aggregate_verify_batch_committee_span_msgtable(detail::ctx(), h_, sigs.data(), table.handle(), idx.data(), ids.data(), n_ids, off.data(),
                                                                               flat.data(), stride, n, res.data(), st.data()));
        if (status) *status = st;
        std::vector<bool> out(n);
        for (size_t i = 0; i < n; i++) out[i] = res[i] != 0;
        return out;
    }
    // AggregateSignature::verify_multiple_aggregate_signatures over a gossip batch whose keys and messages are resident (mbls_verify_multiple_committee_msgtable_rng).
    // A set is a signature, an entry of `table` and either a committee of this table with the participation bits as serialized by SSZ (GossipSet::aggregate) or ONE
    // key of the key table the committees are bound to (GossipSet::single_key: a selection proof, an aggregator's signature, an unaggregated attestation). The same
    // bool as verify_multiple_aggregate_signatures on the spelled-out aggregate keys and messages, rng left in the same state. A committee id, key index or entry
    // index that names nothing throws (DeviceError). rng(): one random byte per call.
    struct GossipSet {
        const AggregateSignature* signature; uint32_t word; Bytes bits; uint32_t msg_index;
        static GossipSet aggregate(const AggregateSignature* sig, uint32_t committee_id, const Bytes& bits, uint32_t msg_index) {
            if (committee_id & MBLS_VM_SET_SINGLE_KEY) throw std::invalid_argument("GossipSet::aggregate: committee ids have 31 bits");
            return GossipSet{sig, committee_id, bits, msg_index};
        }
        static GossipSet single_key(const AggregateSignature* sig, uint32_t key_index, uint32_t msg_index) {
            if (key_index & MBLS_VM_SET_SINGLE_KEY) throw std::invalid_argument("GossipSet::single_key: key indices have 31 bits");
            return GossipSet{sig, MBLS_VM_SET_SINGLE_KEY | key_index, Bytes(), msg_index};
        }
    };
    template <typename Rng>
    bool verify_multiple_aggregate_signatures(Rng&& rng, const std::vector<GossipSet>& sets, const MessageTable& table) const { return vm(rng, sets, table, nullptr); }
    // The same, and in the same call (mbls_verify_multiple_committee_msgtable_locate_rng) which sets of a rejected call are the bad ones, with the semantics of
    // AggregateSignature::verify_multiple_aggregate_signatures_shared_msgs_locate.
    template <typename Rng>
    std::pair<bool, std::vector<bool>> verify_multiple_aggregate_signatures_locate(Rng&& rng, const std::vector<GossipSet>& sets, const MessageTable& table) const {
        std::vector<bool> per_set;
        const bool ok = vm(rng, sets, table, &per_set);
        return {ok, per_set};
    }
    // verify_multiple_aggregate_signatures(rng, batch, table) once per batch of `batches`, in order, as ONE call on the GPU
    // (mbls_verify_multiple_batches_committee_msgtable_rng): one bool per batch, a bad batch rejects itself and nothing else, and the sets of a batch that name one
    // entry of `table` share one Miller loop. rng is left where AggregateSignature::verify_multiple_aggregate_signatures_batches leaves it on the spelled-out sets.
    template <typename Rng>
    std::vector<bool> verify_multiple_aggregate_signatures_batches(Rng&& rng, const std::vector<std::vector<GossipSet>>& batches, const MessageTable& table) const {
        return vm_batches(rng, batches, table, nullptr);
    }
    // The same, and in the same call (mbls_verify_multiple_batches_committee_msgtable_locate_rng) which sets of the rejected batches are the bad ones, with the
    // semantics of AggregateSignature::verify_multiple_aggregate_signatures_batches_locate.
    template <typename Rng>
    std::pair<std::vector<bool>, std::vector<std::vector<bool>>> verify_multiple_aggregate_signatures_batches_locate(
            Rng&& rng, const std::vector<std::vector<GossipSet>>& batches, const MessageTable& table) const {
        std::vector<std::vector<bool>> per_set;
        std::vector<bool> ok = vm_batches(rng, batches, table, &per_set);
        return {ok, per_set};
    }
    // AggregateSignature::verify_multiple_aggregate_signatures over a BLOCK's sets (mbls_verify_multiple_committee_span_msgtable_rng): an attestation names the
    // committees of its committee_bits, in order, with aggregation_bits over their concatenated members (SpanSet::attestation; at most MBLS_SPAN_MAX_COMMITTEES
    // ids -- the sync aggregate is a span of one committee), and a proposer signature, a randao reveal or an exit is under ONE key (SpanSet::single_key). The same
    // bool as verify_multiple_aggregate_signatures on the spelled-out aggregate keys and messages, rng left in the same state. A malformed set, a key index or an
    // entry index that names nothing throws (DeviceError).
    struct SpanSet {
        const AggregateSignature* signature; std::vector<uint32_t> committee_ids; Bytes aggregation_bits; uint32_t msg_index;
        static SpanSet attestation(const AggregateSignature* sig, const std::vector<uint32_t>& committee_ids, const Bytes& aggregation_bits, uint32_t msg_index) {
            for (uint32_t id : committee_ids) if (id & MBLS_VM_SET_SINGLE_KEY) throw std::invalid_argument("SpanSet::attestation: committee ids have 31 bits");
            return SpanSet{sig, committee_ids, aggregation_bits, msg_index};
        }
        static SpanSet single_key(const AggregateSignature* sig, uint32_t key_index, uint32_t msg_index) {
            if (key_index & MBLS_VM_SET_SINGLE_KEY) throw std::invalid_argument("SpanSet::single_key: key indices have 31 bits");
            return SpanSet{sig, {MBLS_VM_SET_SINGLE_KEY | key_index}, Bytes(), msg_index};
        }
    };
    // (the element type is deduced, so that a braced list -- `{}` for no sets -- keeps naming the GossipSet overloads above)
    template <typename Rng, typename Set, typename = typename std::enable_if<std::is_same<Set, SpanSet>::value>::type>
    bool verify_multiple_aggregate_signatures(Rng&& rng, const std::vector<Set>& sets, const MessageTable& table) const { return vm_span(rng, sets, table, nullptr); }
    template <typename Rng, typename Set, typename = typename std::enable_if<std::is_same<Set, SpanSet>::value>::type>
    std::pair<bool, std::vector<bool>> verify_multiple_aggregate_signatures_locate(Rng&& rng, const std::vector<Set>& sets, const MessageTable& table) const {
        std::vector<bool> per_set;
        const bool ok = vm_span(rng, sets, table, &per_set);
        return {ok, per_set};
    }
    // verify_multiple_aggregate_signatures(rng, block, table) over SpanSets once per batch (per block) of `batches`, in order, as ONE call on the GPU
    // (mbls_verify_multiple_batches_committee_span_msgtable_rng): one bool per batch, a bad batch rejects itself and nothing else. rng is left where
    // AggregateSignature::verify_multiple_aggregate_signatures_batches leaves it on the spelled-out sets. A malformed set, a key index or an entry index that
    // names nothing throws (DeviceError).
    template <typename Rng, typename Set, typename = typename std::enable_if<std::is_same<Set, SpanSet>::value>::type>
    std::vector<bool> verify_multiple_aggregate_signatures_batches(Rng&& rng, const std::vector<std::vector<Set>>& batches, const MessageTable& table) const {
        return vm_span_batches(rng, batches, table, nullptr);
    }
    // The same, and in the same call (mbls_verify_multiple_batches_committee_span_msgtable_locate_rng) which sets of the rejected batches are the bad ones.
    template <typename Rng, typename Set, typename = typename std::enable_if<std::is_same<Set, SpanSet>::value>::type>
    std::pair<std::vector<bool>, std::vector<std::vector<bool>>> verify_multiple_aggregate_signatures_batches_locate(
            Rng&& rng, const std::vector<std::vector<Set>>& batches, const MessageTable& table) const {
        std::vector<std::vector<bool>> per_set;
        std::vector<bool> ok = vm_span_batches(rng, batches, table, &per_set);
        return {ok, per_set};
    }
private:
    template <typename Rng>
    std::vector<bool> vm_span_batches(Rng& rng, const std::vector<std::vector<SpanSet>>& batches, const MessageTable& table,
                                      std::vector<std::vector<bool>>* per_set) const {
        if (batches.empty()) return {};
        const size_t nb = batches.size();
        size_t widest = 1;
        for (const auto& b : batches) for (const auto& s : b) widest = std::max(widest, s.aggregation_bits.size());
        const uint32_t stride = uint32_t((widest + 3) / 4 * 4);                         // one stride for every field, a multiple of 4
        Bytes sigs, flat; std::vector<uint32_t> ids, off{0}, idx, boff{0};
        for (const auto& b : batches) {
            for (const SpanSet& s : b) {
                sigs.insert(sigs.end(), s.signature->point.begin(), s.signature->point.end());
                flat.resize(flat.size() + stride, 0);
                std::copy(s.aggregation_bits.begin(), s.aggregation_bits.end(), flat.end() - stride);
                ids.insert(ids.end(), s.committee_ids.begin(), s.committee_ids.end());
                if (ids.size() > 0xFFFFFFFFull) throw std::invalid_argument("verify_multiple_aggregate_signatures_batches: span offsets are 32-bit");
                off.push_back(uint32_t(ids.size())); idx.push_back(s.msg_index);
            }
            if (idx.size() > 0xFFFFFFFEull) throw std::invalid_argument("verify_multiple_aggregate_signatures_batches: set indices are 32-bit");
            boff.push_back(uint32_t(idx.size()));
        }
        const size_t n = idx.size();
        const uint64_t n_ids = ids.size();
        if (ids.empty()) ids.push_back(0);
        using R = typename std::remove_reference<Rng>::type;
        struct src { R* rng; std::exception_ptr err; } u{&rng, nullptr};
        mbls_scalar_source draw = [](void* user, uint64_t* out, uint64_t count) {
            src* p = static_cast<src*>(user);
            try { for (uint64_t i = 0; i < count; i++) out[i] = AggregateSignature::draw_scalar(*p->rng); }
            catch (...) { p->err = std::current_exception(); for (uint64_t i = 0; i < count; i++) out[i] = 0; }        // never unwind through the C frames
        };
        std::vector<uint8_t> res(nb, 0), sres(per_set ? std::max<size_t>(n, 1) : 0, 0);
        const int rc = per_set
            ? mbls_verify_multiple_batches_committee_span_msgtable_locate_rng(detail::ctx(), h_, sigs.data(), ids.data(), n_ids, off.data(), flat.data(), stride,
                                                                              table.handle(), idx.data(), n, boff.data(), 0, nb, res.data(), sres.data(), nullptr, draw, &u)
            : mbls_verify_multiple_batches_committee_span_msgtable_rng(detail::ctx(), h_, sigs.data(), ids.data(), n_ids, off.data(), flat.data(), stride, table.handle(),
                                                                       idx.data(), n, boff.data(), 0, nb, res.data(), draw, &u);
        if (u.err) std::rethrow_exception(u.err);
        detail::check(rc);
        if (per_set) {
            per_set->clear();
            for (size_t b = 0; b < nb; b++) per_set->emplace_back(sres.begin() + boff[b], sres.begin() + boff[b + 1]);
        }
        return std::vector<bool>(res.begin(), res.end());
    }
    template <typename Rng>
    bool vm_span(Rng& rng, const std::vector<SpanSet>& sets, const MessageTable& table, std::vector<bool>* per_set) const {
        if (sets.empty()) return true;
        const size_t n = sets.size();
        size_t widest = 1;
        for (const auto& s : sets) widest = std::max(widest, s.aggregation_bits.size());
        const uint32_t stride = uint32_t((widest + 3) / 4 * 4);                         // one stride for every field, a multiple of 4
        Bytes sigs, flat(size_t(stride) * n, 0); std::vector<uint32_t> ids, off{0}, idx;
        for (size_t i = 0; i < n; i++) {
            const SpanSet& s = sets[i];
            sigs.insert(sigs.end(), s.signature->point.begin(), s.signature->point.end());
            std::copy(s.aggregation_bits.begin(), s.aggregation_bits.end(), flat.begin() + size_t(stride) * i);
            ids.insert(ids.end(), s.committee_ids.begin(), s.committee_ids.end());
            if (ids.size() > 0xFFFFFFFFull) throw std::invalid_argument("verify_multiple_aggregate_signatures: span offsets are 32-bit");
            off.push_back(uint32_t(ids.size())); idx.push_back(s.msg_index);
        }
        const uint64_t n_ids = ids.size();
        if (ids.empty()) ids.push_back(0);
        using R = typename std::remove_reference<Rng>::type;
        struct src { R* rng; std::exception_ptr err; } u{&rng, nullptr};
        mbls_scalar_source draw = [](void* user, uint64_t* out, uint64_t count) {
            src* p = static_cast<src*>(user);
            try { for (uint64_t i = 0; i < count; i++) out[i] = AggregateSignature::draw_scalar(*p->rng); }
            catch (...) { p->err = std::current_exception(); for (uint64_t i = 0; i < count; i++) out[i] = 0; }        // never unwind through the C frames
        };
        uint8_t ok = 0;
        std::vector<uint8_t> sres(per_set ? n : 0);
        const int rc = per_set
            ? mbls_verify_multiple_committee_span_msgtable_locate_rng(detail::ctx(), h_, sigs.data(), ids.data(), n_ids, off.data(), flat.data(), stride, table.handle(),
                                                                      idx.data(), n, &ok, sres.data(), nullptr, draw, &u)
            : mbls_verify_multiple_committee_span_msgtable_rng(detail::ctx(), h_, sigs.data(), ids.data(), n_ids, off.data(), flat.data(), stride, table.handle(), idx.data(),
                                                               n, &ok, draw, &u);
        if (u.err) std::rethrow_exception(u.err);
        detail::check(rc);
        if (per_set) per_set->assign(sres.begin(), sres.end());
        return ok == 1;
    }
    template <typename Rng>
    std::vector<bool> vm_batches(Rng& rng, const std::vector<std::vector<GossipSet>>& batches, const MessageTable& table, std::vector<std::vector<bool>>* per_set) const {
        if (batches.empty()) return {};
        const size_t nb = batches.size();
        const size_t covering = (size_t(max_members()) + 7) / 8;
        const uint32_t stride = uint32_t(((covering ? covering : 1) + 3) / 4 * 4);
        Bytes sigs, flat; std::vector<uint32_t> words, idx, boff{0};
        for (const auto& b : batches) {
            for (const GossipSet& s : b) {
                sigs.insert(sigs.end(), s.signature->point.begin(), s.signature->point.end());
                flat.resize(flat.size() + stride, 0);
                std::copy(s.bits.begin(), s.bits.begin() + std::min(s.bits.size(), size_t(stride)), flat.end() - stride);
                words.push_back(s.word); idx.push_back(s.msg_index);
            }
            if (words.size() > 0xFFFFFFFEull) throw std::invalid_argument("verify_multiple_aggregate_signatures_batches: set indices are 32-bit");
            boff.push_back(uint32_t(words.size()));
        }
        const size_t n = words.size();
        using R = typename std::remove_reference<Rng>::type;
        struct src { R* rng; std::exception_ptr err; } u{&rng, nullptr};
        mbls_scalar_source draw = [](void* user, uint64_t* out, uint64_t count) {
            src* p = static_cast<src*>(user);
            try { for (uint64_t i = 0; i < count; i++) out[i] = AggregateSignature::draw_scalar(*p->rng); }
            catch (...) { p->err = std::current_exception(); for (uint64_t i = 0; i < count; i++) out[i] = 0; }        // never unwind through the C frames
        };
        std::vector<uint8_t> res(nb, 0), sres(per_set ? std::max<size_t>(n, 1) : 0, 0);
        const int rc = per_set
            ? mbls_verify_multiple_batches_committee_msgtable_locate_rng(detail::ctx(), h_, sigs.data(), words.data(), flat.data(), stride, table.handle(), idx.data(), n,
                                                                         boff.data(), 0, nb, res.data(), sres.data(), nullptr, draw, &u)
            : mbls_verify_multiple_batches_committee_msgtable_rng(detail::ctx(), h_, sigs.data(), words.data(), flat.data(), stride, table.handle(), idx.data(), n,
                                                                  boff.data(), 0, nb, res.data(), draw, &u);
        if (u.err) std::rethrow_exception(u.err);
        detail::check(rc);
        if (per_set) {
            per_set->clear();
            for (size_t b = 0; b < nb; b++) per_set->emplace_back(sres.begin() + boff[b], sres.begin() + boff[b + 1]);
        }
        return std::vector<bool>(res.begin(), res.end());
    }
    template <typename Rng>
    bool vm(Rng& rng, const std::vector<GossipSet>& sets, const MessageTable& table, std::vector<bool>* per_set) const {
        if (sets.empty()) return true;
        const size_t n = sets.size();
        const size_t covering = (size_t(max_members()) + 7) / 8;                   // one stride for every field, as fast_aggregate_verify_batch_committee_msgtable lays them out
        const uint32_t stride = uint32_t(((covering ? covering : 1) + 3) / 4 * 4);
        Bytes sigs, flat(size_t(stride) * n, 0); std::vector<uint32_t> words, idx;
        for (size_t i = 0; i < n; i++) {
            const GossipSet& s = sets[i];
            sigs.insert(sigs.end(), s.signature->point.begin(), s.signature->point.end());
            std::copy(s.bits.begin(), s.bits.begin() + std::min(s.bits.size(), size_t(stride)), flat.begin() + size_t(stride) * i);
            words.push_back(s.word); idx.push_back(s.msg_index);
        }
        using R = typename std::remove_reference<Rng>::type;
        struct src { R* rng; std::exception_ptr err; } u{&rng, nullptr};
        mbls_scalar_source draw = [](void* user, uint64_t* out, uint64_t count) {
            src* p = static_cast<src*>(user);
            try { for (uint64_t i = 0; i < count; i++) out[i] = AggregateSignature::draw_scalar(*p->rng); }
            catch (...) { p->err = std::current_exception(); for (uint64_t i = 0; i < count; i++) out[i] = 0; }        // never unwind through the C frames
        };
        uint8_t ok = 0;
        std::vector<uint8_t> sres(per_set ? n : 0);
        const int rc = per_set
            ? mbls_verify_multiple_committee_msgtable_locate_rng(detail::ctx(), h_, sigs.data(), words.data(), flat.data(), stride, table.handle(), idx.data(), n, &ok,
                                                                 sres.data(), nullptr, draw, &u)
            : mbls_verify_multiple_committee_msgtable_rng(detail::ctx(), h_, sigs.data(), words.data(), flat.data(), stride, table.handle(), idx.data(), n, &ok, draw, &u);
        if (u.err) std::rethrow_exception(u.err);
        detail::check(rc);
        if (per_set) per_set->assign(sres.begin(), sres.end());
        return ok == 1;
    }
};
// n x AggregateSignature::fast_aggregate_verify over a committee table and a resident message table (mbls_fast_aggregate_verify_batch_committee_msgtable): item i =
// (sigs[i], entry msg_idx[i], the members of committee cmt_idx[i] whose bit is set in bits[i]); the fields are laid out at one stride (16 bytes for 128 members)
inline std::vector<bool> fast_aggregate_verify_batch_committee_msgtable(const CommitteeTable& committees, const std::vector<AggregateSignature>& sigs, const MessageTable& table,
                                                                        const std::vector<uint32_t>& msg_idx, const std::vector<uint32_t>& cmt_idx,
                                                                        const std::vector<Bytes>& bits) {
    const size_t n = sigs.size();
    if (msg_idx.size() != n || cmt_idx.size() != n || bits.size() != n)
        throw std::invalid_argument("fast_aggregate_verify_batch_committee_msgtable: one message index, one committee id and one bitfield per signature");
    // one stride for every field: the bytes that cover the table's largest committee, rounded up to 4 (bytes of a field beyond that hold only bits at or above
    // every committee's size, which the entry ignores)
    const size_t covering = (size_t(committees.max_members()) + 7) / 8;
    const uint32_t stride = uint32_t(((covering ? covering : 1) + 3) / 4 * 4);
    Bytes s, flat(size_t(stride) * (n ? n : 1), 0);
    for (size_t i = 0; i < n; i++) {
        s.insert(s.end(), sigs[i].point.begin(), sigs[i].point.end());
        std::copy(bits[i].begin(), bits[i].begin() + std::min(bits[i].size(), size_t(stride)), flat.begin() + size_t(stride) * i);
    }
    std::vector<uint8_t> res(n ? n : 1);
    detail::check(mbls_fast_aggregate_verify_batch_committee_msgtable(detail::ctx(), committees.handle(), s.data(), table.handle(), msg_idx.data(), cmt_idx.data(), flat.data(),
                                                                      stride, n, res.data(), nullptr));
    std::vector<bool> out(n);
    for (size_t i = 0; i < n; i++) out[i] = res[i] == 1;
    return out;
}

class MultiGpu {
    mbls_multi* h_ = nullptr;
public:
    explicit MultiGpu(const std::vector<int>& device_ids) {
        if (mbls_multi_create(&h_, device_ids.data(), int(device_ids.size())) != MBLS_OK) throw DeviceError("mbls_multi_create failed");
    }
    MultiGpu(const MultiGpu&) = delete; MultiGpu& operator=(const MultiGpu&) = delete;
    ~MultiGpu() { mbls_multi_destroy(h_); }
    int devices() const { return mbls_multi_device_count(h_); }
    // the handle's exchange steps as RCCL all-gathers between the devices (true) or through host memory (false; exchange_note() says why)
    bool rccl_active() const { return mbls_multi_rccl_active(h_) == 1; }
    std::string exchange_note() const { return mbls_multi_exchange_note(h_); }
    mbls_multi* handle() const { return h_; }
    // n x fast_aggregate_verify with the results as one packed accept bitmap that every device ends up holding (bit i % 64 of word i / 64 = item i)
    std::vector<uint64_t> fast_aggregate_verify_bitmap(const std::vector<AggregateSignature>& sigs, const std::vector<Bytes>& msgs, const std::vector<std::vector<const PublicKey*>>& keys) const {
        const size_t n = sigs.size();
        if (msgs.size() != n || keys.size() != n) throw std::invalid_argument("one message and one key set per signature");
        Bytes s, m, p; std::vector<uint64_t> moff{0}; std::vector<uint32_t> koff{0};
        for (size_t i = 0; i < n; i++) {
            s.insert(s.end(), sigs[i].point.begin(), sigs[i].point.end());
            m.insert(m.end(), msgs[i].begin(), msgs[i].end()); moff.push_back(m.size());
            for (auto* k : keys[i]) p.insert(p.end(), k->point.begin(), k->point.end());
            if (p.size() / 96 > 0xFFFFFFFFull) throw std::invalid_argument("fast_aggregate_verify_bitmap: key indices are 32-bit");
            koff.push_back(uint32_t(p.size() / 96));
        }
        std::vector<uint64_t> words((n + 63) / 64 ? (n + 63) / 64 : 1);
        int rc = mbls_multi_fast_aggregate_verify_bitmap(h_, s.data(), m.data(), 0, moff.data(), p.data(), MBLS_PK_UNCOMPRESSED, koff.data(), n, 0, words.data(), nullptr);
        if (rc != MBLS_OK) throw DeviceError(std::string("mbls_multi: ") + mbls_multi_last_error(h_));
        words.resize((n + 63) / 64);
        return words;
    }
    // n x AggregateSignature::fast_aggregate_verify; messages of any length each
    std::vector<bool> fast_aggregate_verify(const std::vector<AggregateSignature>& sigs, const std::vector<Bytes>& msgs, const std::vector<std::vector<const PublicKey*>>& keys) const {
        const size_t n = sigs.size();
        if (msgs.size() != n || keys.size() != n) throw std::invalid_argument("one message and one key set per signature");
        Bytes s, m, p; std::vector<uint64_t> moff{0}; std::vector<uint32_t> koff{0};
        for (size_t i = 0; i < n; i++) {
            s.insert(s.end(), sigs[i].point.begin(), sigs[i].point.end());
            m.insert(m.end(), msgs[i].begin(), msgs[i].end()); moff.push_back(m.size());
            for (auto* k : keys[i]) p.insert(p.end(), k->point.begin(), k->point.end());
            if (p.size() / 96 > 0xFFFFFFFFull) throw std::invalid_argument("fast_aggregate_verify: key indices are 32-bit");
            koff.push_back(uint32_t(p.size() / 96));
        }
        std::vector<uint8_t> res(n ? n : 1);
        int rc = mbls_multi_fast_aggregate_verify_batch(h_, s.data(), m.data(), 0, moff.data(), p.data(), MBLS_PK_UNCOMPRESSED, koff.data(), n, 0, res.data(), nullptr);
        if (rc != MBLS_OK) throw DeviceError(std::string("mbls_multi: ") + mbls_multi_last_error(h_));
        return std::vector<bool>(res.begin(), res.begin() + n);
    }
};


// A verification stream on the library's context (include/mbls.h, "verification stream"): calls of any size are packed into full-round
// launches. submit() takes the same objects as MultiGpu::fast_aggregate_verify and returns a ticket; Ticket::get() waits for the call.
// The stream keeps every call's staged inputs until the call completes; destroying it completes every pending call.
class VerifyStream {
    struct Call { Bytes s, m, p; std::vector<uint64_t> moff; std::vector<uint32_t> koff, midx; std::vector<uint8_t> res; uint64_t ticket = 0; size_t n = 0; };
    mbls_stream* h_ = nullptr;
    uint32_t bits_stride_ = 0;               // a committee stream's (Call: the ids travel in koff, the fields in p)
    std::mutex mu_;
    std::deque<std::shared_ptr<Call>> live_;
    void check(int rc) const { if (rc != MBLS_OK) throw DeviceError(std::string("mbls_stream: ") + mbls_stream_last_error(h_)); }
public:
    class Ticket {
        VerifyStream* vs_; std::shared_ptr<Call> c_;
    public:
        Ticket(VerifyStream* vs, std::shared_ptr<Call> c) : vs_(vs), c_(std::move(c)) {}
        uint64_t id() const { return c_->ticket; }
        bool ready() const { return mbls_stream_query(vs_->h_, c_->ticket) != MBLS_PENDING; }
        std::vector<bool> get() const { vs_->wait(c_->ticket); return std::vector<bool>(c_->res.begin(), c_->res.begin() + c_->n); }
    };
    // policy: MBLS_STREAM_WORK_CONSERVING or MBLS_STREAM_FULL_ROUNDS; round_items 0 = the device's round
    explicit VerifyStream(uint32_t policy = MBLS_STREAM_WORK_CONSERVING, uint64_t round_items = 0) {
        mbls_stream_opts o{}; o.round_items = round_items; o.policy = policy;
        if (mbls_stream_create(detail::ctx(), MBLS_STREAM_FAST_AGGREGATE_VERIFY, MBLS_PK_UNCOMPRESSED, nullptr, &o, &h_) != MBLS_OK)
            throw DeviceError(std::string("mbls_stream_create: ") + mbls_last_error(detail::ctx()));
    }
    // a stream over a resident message table: its calls name their messages by table index (the submit overload below); destroy it before the table
    explicit VerifyStream(MessageTable& table, uint32_t policy = MBLS_STREAM_WORK_CONSERVING, uint64_t round_items = 0) {
        mbls_stream_opts o{}; o.round_items = round_items; o.policy = policy;
        if (mbls_stream_create_msgtable(detail::ctx(), MBLS_STREAM_FAST_AGGREGATE_VERIFY, MBLS_PK_UNCOMPRESSED, nullptr, table.handle(), &o, &h_) != MBLS_OK)
            throw DeviceError(std::string("mbls_stream_create_msgtable: ") + mbls_last_error(detail::ctx()));
    }
    // a stream over a committee table and a message table (mbls_stream_create_committee): its calls name a committee and an entry per item and carry the
    // participation bits (submit_committee below). bits_stride: a multiple of 4 whose 8 x covers the table's largest committee, now and for every later append.
    // Destroy the stream before both tables.
    VerifyStream(CommitteeTable& committees, MessageTable& table, uint32_t bits_stride, uint32_t policy = MBLS_STREAM_WORK_CONSERVING, uint64_t round_items = 0)
        : bits_stride_(bits_stride) {
        mbls_stream_opts o{}; o.round_items = round_items; o.policy = policy;
        if (mbls_stream_create_committee(detail::ctx(), committees.handle(), table.handle(), bits_stride, &o, &h_) != MBLS_OK)
            throw DeviceError(std::string("mbls_stream_create_committee: ") + mbls_last_error(detail::ctx()));
    }
    VerifyStream(const VerifyStream&) = delete; VerifyStream& operator=(const VerifyStream&) = delete;
    ~VerifyStream() { mbls_stream_destroy(h_); }
    mbls_stream* handle() const { return h_; }
    // n x AggregateSignature::fast_aggregate_verify; messages of any length each
    Ticket submit(const std::vector<AggregateSignature>& sigs, const std::vector<Bytes>& msgs, const std::vector<std::vector<const PublicKey*>>& keys) {
        const size_t n = sigs.size();
        if (n == 0 || msgs.size() != n || keys.size() != n) throw std::invalid_argument("one message and one key set per signature, at least one item");
        auto c = std::make_shared<Call>();
        c->moff.push_back(0); c->koff.push_back(0); c->n = n; c->res.resize(n);
        for (size_t i = 0; i < n; i++) {
            c->s.insert(c->s.end(), sigs[i].point.begin(), sigs[i].point.end());
            c->m.insert(c->m.end(), msgs[i].begin(), msgs[i].end()); c->moff.push_back(c->m.size());
            for (auto* k : keys[i]) c->p.insert(c->p.end(), k->point.begin(), k->point.end());
            if (c->p.size() / 96 > 0xFFFFFFFFull) throw std::invalid_argument("VerifyStream::submit: key offsets are 32-bit");
            c->koff.push_back(uint32_t(c->p.size() / 96));
        }
        std::lock_guard<std::mutex> g(mu_);
        while (!live_.empty() && mbls_stream_query(h_, live_.front()->ticket) != MBLS_PENDING) live_.pop_front();
        check(mbls_stream_submit(h_, c->s.data(), c->m.data(), 0, c->moff.data(), c->p.data(), nullptr, c->koff.data(), n, 0, c->res.data(), nullptr, &c->ticket));
        live_.push_back(c);
        return Ticket(this, c);
    }
    // the same over the stream's message table: item i's message is entry msg_idx[i] (an index the table does not hold when the call's round launches rejects
    // its item). Only on a stream made over a MessageTable; the overload above only on one that was not.
    Ticket submit(const std::vector<AggregateSignature>& sigs, const std::vector<uint32_t>& msg_idx, const std::vector<std::vector<const PublicKey*>>& keys) {
        const size_t n = sigs.size();
        if (n == 0 || msg_idx.size() != n || keys.size() != n) throw std::invalid_argument("one message index and one key set per signature, at least one item");
        auto c = std::make_shared<Call>();
        c->koff.push_back(0); c->n = n; c->res.resize(n); c->midx = msg_idx;
        for (size_t i = 0; i < n; i++) {
            c->s.insert(c->s.end(), sigs[i].point.begin(), sigs[i].point.end());
            for (auto* k : keys[i]) c->p.insert(c->p.end(), k->point.begin(), k->point.end());
            if (c->p.size() / 96 > 0xFFFFFFFFull) throw std::invalid_argument("VerifyStream::submit: key offsets are 32-bit");
            c->koff.push_back(uint32_t(c->p.size() / 96));
        }
        std::lock_guard<std::mutex> g(mu_);
        while (!live_.empty() && mbls_stream_query(h_, live_.front()->ticket) != MBLS_PENDING) live_.pop_front();
        check(mbls_stream_submit_msgidx(h_, c->s.data(), c->midx.data(), c->p.data(), nullptr, c->koff.data(), n, 0, c->res.data(), nullptr, &c->ticket));
        live_.push_back(c);
        return Ticket(this, c);
    }
    // a committee stream's call: item i is signature i over entry msg_idx[i] by the members of committee cmt_idx[i] whose bit is set in fields[i] (SSZ bit order, a
    // Bitlist's delimiter may stay). The fields of ONE call travel at one length -- the longest of them, shorter ones zero-extended --, which may differ from call
    // to call and need not be a multiple of 4; it must not exceed the stream's bits_stride. An id or an entry index that names nothing rejects its item. status,
    // when given, receives the items' MBLS_ST_* words once the ticket is done (it must stay valid until then).
    Ticket submit_committee(const std::vector<AggregateSignature>& sigs, const std::vector<uint32_t>& msg_idx, const std::vector<uint32_t>& cmt_idx,
                            const std::vector<Bytes>& fields, std::vector<uint32_t>* status = nullptr) {
        const size_t n = sigs.size();
        if (n == 0 || msg_idx.size() != n || cmt_idx.size() != n || fields.size() != n)
            throw std::invalid_argument("one message index, one committee id and one field per signature, at least one item");
        size_t len = 1;
        for (const auto& f : fields) len = std::max(len, f.size());
        if (len > bits_stride_) throw std::invalid_argument("VerifyStream::submit_committee: a field is longer than the stream's bits_stride");
        auto c = std::make_shared<Call>();
        c->n = n; c->res.resize(n); c->midx = msg_idx; c->koff = cmt_idx; c->p.assign(len * n, 0);
        for (size_t i = 0; i < n; i++) {
            c->s.insert(c->s.end(), sigs[i].point.begin(), sigs[i].point.end());
            std::copy(fields[i].begin(), fields[i].end(), c->p.begin() + len * i);
        }
        if (status) status->assign(n, 0);
        std::lock_guard<std::mutex> g(mu_);
        while (!live_.empty() && mbls_stream_query(h_, live_.front()->ticket) != MBLS_PENDING) live_.pop_front();
        check(mbls_stream_submit_committee(h_, c->s.data(), c->midx.data(), c->koff.data(), c->p.data(), uint32_t(len), n, c->res.data(), status ? status->data() : nullptr,
                                           &c->ticket));
        live_.push_back(c);
        return Ticket(this, c);
    }
    void flush() { check(mbls_stream_flush(h_)); }
    void wait(uint64_t ticket) const { check(mbls_stream_wait(h_, ticket)); }
    mbls_stream_stats stats() const { mbls_stream_stats st{}; check(mbls_stream_get_stats(h_, &st)); return st; }
};

// A verify_multiple stream over a committee table and a message table (include/mbls.h, mbls_stream_create_vm_committee): the gossip caller, many threads each
// holding ONE small batch. A call is one batch of CommitteeTable::GossipSet and is never split; the stream packs the batches of many callers into one call of
// mbls_verify_multiple_batches_committee_msgtable_locate_device per round and answers per batch and per set. submit() draws one scalar per set from rng AT
// SUBMIT, in set order, by the reference's rule (AggregateSignature::draw_scalar) -- the one difference from the _rng entries: nothing is read back before the
// draw, so a batch with a signature outside G2 still consumes a scalar for every set. Destroy the stream before both tables.
class VerifyMultipleStream {
    struct Call { Bytes s, f; std::vector<uint32_t> words, midx, sst; std::vector<uint64_t> rands; std::vector<uint8_t> sres; uint8_t res = 0; uint32_t st = 0;
                  uint64_t ticket = 0; size_t n = 0; };
    mbls_stream* h_ = nullptr;
    uint32_t bits_stride_ = 0;
    std::mutex mu_;
    std::deque<std::shared_ptr<Call>> live_;
    void check(int rc) const { if (rc != MBLS_OK) throw DeviceError(std::string("mbls_stream: ") + mbls_stream_last_error(h_)); }
public:
    class Ticket {
        VerifyMultipleStream* vs_; std::shared_ptr<Call> c_;
    public:
        Ticket(VerifyMultipleStream* vs, std::shared_ptr<Call> c) : vs_(vs), c_(std::move(c)) {}
        uint64_t id() const { return c_->ticket; }
        bool ready() const { return mbls_stream_query(vs_->h_, c_->ticket) != MBLS_PENDING; }
        // the batch's bool, and which sets of a rejected batch are the good ones (every set of an accepted batch: true)
        std::pair<bool, std::vector<bool>> get() const { vs_->wait(c_->ticket); return {c_->res == 1, std::vector<bool>(c_->sres.begin(), c_->sres.end())}; }
        // the batch's MBLS_ST_* word and the sets' words, once the call is done
        std::pair<uint32_t, std::vector<uint32_t>> status() const { vs_->wait(c_->ticket); return {c_->st, c_->sst}; }
    };
    // bits_stride: a multiple of 4 whose 8 x covers the table's largest committee, now and for every later append; round_items 0 = the device's round
    VerifyMultipleStream(CommitteeTable& committees, MessageTable& table, uint32_t bits_stride, uint32_t policy = MBLS_STREAM_WORK_CONSERVING, uint64_t round_items = 0)
        : bits_stride_(bits_stride) {
        mbls_stream_opts o{}; o.round_items = round_items; o.policy = policy;
        if (mbls_stream_create_vm_committee(detail::ctx(), committees.handle(), table.handle(), bits_stride, &o, &h_) != MBLS_OK)
            throw DeviceError(std::string("mbls_stream_create_vm_committee: ") + mbls_last_error(detail::ctx()));
    }
    VerifyMultipleStream(const VerifyMultipleStream&) = delete; VerifyMultipleStream& operator=(const VerifyMultipleStream&) = delete;
    ~VerifyMultipleStream() { mbls_stream_destroy(h_); }
    mbls_stream* handle() const { return h_; }
    // one batch: at least one set and fewer than round_items of them. The fields travel at the length of the longest (a batch of single-key sets only: 0 bytes),
    // which must not exceed the stream's bits_stride. A committee id, key index or entry index that names nothing rejects the batch and names its set.
    template <typename Rng>
    Ticket submit(Rng&& rng, const std::vector<CommitteeTable::GossipSet>& sets) {
        const size_t n = sets.size();
        if (n == 0) throw std::invalid_argument("VerifyMultipleStream::submit: a batch holds at least one set");
        size_t len = 0;
        for (const auto& s : sets) len = std::max(len, s.bits.size());
        if (len > bits_stride_) throw std::invalid_argument("VerifyMultipleStream::submit: a field is longer than the stream's bits_stride");
        auto c = std::make_shared<Call>();
        c->n = n; c->sres.assign(n, 0); c->sst.assign(n, 0); c->f.assign(len * n, 0);
        for (size_t i = 0; i < n; i++) {
            c->s.insert(c->s.end(), sets[i].signature->point.begin(), sets[i].signature->point.end());
            std::copy(sets[i].bits.begin(), sets[i].bits.end(), c->f.begin() + len * i);
            c->words.push_back(sets[i].word); c->midx.push_back(sets[i].msg_index);
            c->rands.push_back(AggregateSignature::draw_scalar(rng));
        }
        std::lock_guard<std::mutex> g(mu_);
        while (!live_.empty() && mbls_stream_query(h_, live_.front()->ticket) != MBLS_PENDING) live_.pop_front();
        check(mbls_stream_submit_vm(h_, c->s.data(), c->words.data(), len ? c->f.data() : nullptr, uint32_t(len), c->midx.data(), c->rands.data(), n, &c->res, &c->st,
                                    c->sres.data(), c->sst.data(), &c->ticket));
        live_.push_back(c);
        return Ticket(this, c);
    }
    void flush() { check(mbls_stream_flush(h_)); }
    void wait(uint64_t ticket) const { check(mbls_stream_wait(h_, ticket)); }
    mbls_stream_stats stats() const { mbls_stream_stats st{}; check(mbls_stream_get_stats(h_, &st)); return st; }
};
}  // namespace milagro_bls

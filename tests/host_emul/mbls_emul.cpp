// mbls_emul.cpp -- TEST INFRASTRUCTURE: compiles the lane bodies of the HIP kernels
// (milagro_bls_amd/csrc/mbls_*.h) as plain C++ and runs them one "lane" at a time on the CPU, so the
// CPU-only test suite can check every phase against the oracle before a GPU is involved. It is not a
// fallback: the product library (libmbls_hip.so) contains no CPU path and never loads this file.
#define MBLS_HOST_EMUL 1
#include <stdlib.h>
#include <string.h>
#include "../../milagro_bls_amd/csrc/mbls_ops.h"

static uint64_t emul_phase_ops[5];
extern "C" {
void emul_op_counts(uint64_t* mul, uint64_t* sqr, int reset) { *mul = mbls_cnt_mul; *sqr = mbls_cnt_sqr; if (reset) mbls_cnt_mul = mbls_cnt_sqr = 0; }
// the full fast_aggregate_verify / verify pipeline over n items, same phases and workspace layout as the GPU
void emul_verify_batch(const uint8_t* sigs, const uint8_t* msgs, uint32_t mlen, const uint8_t* pks, int fmt,
                       const uint32_t* offsets, uint64_t n, uint32_t k, int mode, uint8_t* results, uint32_t* status) {
    mbls_ws ws; ws.stride = n ? n : 1; ws.w = (uint32_t*)calloc((size_t)MBLS_SLOT_COUNT * 12 * ws.stride, 4);
    const uint32_t pkb = fmt == MBLS_PK_COMPRESSED ? 48 : 96;
    if (fmt == MBLS_PK_COMPRESSED && !offsets && k > 1) {   // staged path: lane per key, then per-item sums (as on the GPU)
        uint32_t* xy = (uint32_t*)malloc((size_t)n * k * 96); uint8_t* fl = (uint8_t*)malloc((size_t)n * k);
        for (uint64_t j = 0; j < n * k; j++) lane_pk_decompress(j, pks, xy, fl);
        for (uint64_t i = 0; i < n; i++) lane_aggregate_decoded(ws, i, xy + 24 * (uint64_t)k * i, fl + (uint64_t)k * i, k, mode, &status[i]);
        free(xy); free(fl);
    } else
    for (uint64_t i = 0; i < n; i++) {
        uint64_t first = offsets ? offsets[i] : (uint64_t)k * i; uint32_t cnt = offsets ? offsets[i + 1] - offsets[i] : k;
        lane_aggregate(ws, i, pks + pkb * first, cnt, fmt, mode, &status[i]);
    }
    emul_phase_ops[0] = mbls_cnt_mul + mbls_cnt_sqr;
    for (uint64_t i = 0; i < n; i++) lane_sig(ws, i, sigs + 96 * i, &status[i]);
    emul_phase_ops[1] = mbls_cnt_mul + mbls_cnt_sqr;
    for (uint64_t i = 0; i < n; i++) lane_hash(ws, i, msgs + (uint64_t)mlen * i, mlen);
    emul_phase_ops[2] = mbls_cnt_mul + mbls_cnt_sqr;
    for (uint64_t i = 0; i < n; i++) lane_miller(ws, i);
    emul_phase_ops[3] = mbls_cnt_mul + mbls_cnt_sqr;
    for (uint64_t i = 0; i < n; i++) lane_final(ws, i, &status[i], &results[i]);
    emul_phase_ops[4] = mbls_cnt_mul + mbls_cnt_sqr;
    free(ws.w);
}
void emul_phase_counts(uint64_t out[5]) { for (int i = 0; i < 5; i++) out[i] = emul_phase_ops[i]; }
void emul_g1_decode(const uint8_t* in, int fmt, int validate, uint64_t n, uint8_t* out96, uint8_t* err) { for (uint64_t i = 0; i < n; i++) op_g1_decode(i, in, fmt, validate, out96, err); }
void emul_g1_key_validate(const uint8_t* in96, uint64_t n, uint8_t* ok) { for (uint64_t i = 0; i < n; i++) op_g1_key_validate(i, in96, ok); }
void emul_g1_compress(const uint8_t* in96, uint64_t n, uint8_t* out48, uint8_t* err) { for (uint64_t i = 0; i < n; i++) op_g1_compress(i, in96, out48, err); }
void emul_g2_check(const uint8_t* in96, uint64_t n, uint8_t* err, uint8_t* in_g2) { for (uint64_t i = 0; i < n; i++) op_g2_check(i, in96, err, in_g2); }
void emul_g2_add(const uint8_t* a, const uint8_t* b, uint64_t n, uint8_t* out, uint8_t* err) { for (uint64_t i = 0; i < n; i++) op_g2_add(i, a, b, out, err); }
void emul_g1_add(const uint8_t* a, const uint8_t* b, uint64_t n, uint8_t* out, uint8_t* err) { for (uint64_t i = 0; i < n; i++) op_g1_add(i, a, b, out, err); }
void emul_sign(const uint8_t* sks, const uint8_t* msgs, uint32_t mlen, uint64_t n, uint8_t* out96) { for (uint64_t i = 0; i < n; i++) op_sign(i, sks, msgs, mlen, out96); }
void emul_sk_to_pk(const uint8_t* sks, int fmt, uint64_t n, uint8_t* out) { for (uint64_t i = 0; i < n; i++) op_sk_to_pk(i, sks, fmt, out); }
void emul_hash_to_g2(const uint8_t* msgs, uint32_t mlen, uint64_t n, uint8_t* out96) { for (uint64_t i = 0; i < n; i++) op_hash_to_g2(i, msgs, mlen, out96); }
// hash_to_field through the register-only function the hashing kernel uses (out: 4 x 12 words per item: u0.c0, u0.c1, u1.c0, u1.c1)
// and through expand_message_xmd_256 + fp_from_two_digests (out_ref)
void emul_hash_fields(const uint8_t* msgs, uint32_t mlen, uint64_t n, uint32_t* out, uint32_t* out_ref) {
    mbls_ws ws; ws.stride = n ? n : 1; ws.w = (uint32_t*)calloc((size_t)49 * 12 * ws.stride, 4);
    for (uint64_t i = 0; i < n; i++) {
        hash_fields_to_ws(ws.w, ws.stride, i, msgs + (uint64_t)mlen * i, mlen);
        const int slot[4] = {31, 32, 37, 38};
        for (int q = 0; q < 4; q++) { fp v = ws_ld(ws, slot[q], i); for (int j = 0; j < 12; j++) out[(4 * i + q) * 12 + j] = v[j]; }
        uint32_t ub[64];
        expand_message_xmd_256(ub, msgs + (uint64_t)mlen * i, mlen, MBLS_DST_POP, MBLS_DST_POP_LEN);
        for (int q = 0; q < 4; q++) { fp v = fp_from_two_digests(ub + 16 * q, ub + 16 * q + 8); for (int j = 0; j < 12; j++) out_ref[(4 * i + q) * 12 + j] = v[j]; }
    }
    free(ws.w);
}
// hash_to_curve_g2 after hash_to_field on caller-supplied field elements (the compiled body mbls_map_to_g2_probe runs in mode 0):
// u192 = n x (u0.c0, u0.c1, u1.c0, u1.c1), canonical 48-byte big-endian values; compressed output
void emul_map_to_g2(const uint8_t* u192, uint64_t n, uint8_t* out96) {
    for (uint64_t i = 0; i < n; i++) {
        fp2 u[2];
        for (int e = 0; e < 2; e++) {
            u[e].c0 = fp_to_mont(fp_raw_from_be(u192 + 192 * i + 96 * e)); u[e].c1 = fp_to_mont(fp_raw_from_be(u192 + 192 * i + 96 * e + 48));
        }
        g2j q0, q1, h; map_to_curve_g2(&q0, &u[0]); map_to_curve_g2(&q1, &u[1]);
        g2_add(&q0, &q0, &q1); g2_clear_cofactor(&h, &q0);
        g2_encode_jacobian(out96 + 96 * i, &h);
    }
}
// the compiled two-pair Miller loop (lane_miller without LDS: what mbls_miller_probe runs in mode 0) on caller-supplied operands: in624 = n x (apk X, Y, Z;
// sig x.c0, x.c1, y.c0, y.c1 with y = 0 for infinity; H X.c0 .. Z.c1), canonical 48-byte big-endian values; out576 = the 12 coefficients of f in the order of
// slot F. one_pair != 0: f(H, apk) alone through miller_loop(.., 1), the compiled statement of what the one-pair routines compute.
void emul_miller(const uint8_t* in624, uint64_t n, uint8_t* out576, int one_pair) {
    mbls_ws ws; ws.stride = 1; ws.w = (uint32_t*)calloc((size_t)MBLS_SLOT_COUNT * 12, 4);
    for (uint64_t i = 0; i < n; i++) {
        for (int k = 0; k < 13; k++) ws_st(ws, k, 0, fp_to_mont(fp_raw_from_be(in624 + 624 * i + 48 * k)));      // slots APK 0..2, SIG 3..6, H 7..12
        if (one_pair) {
            g2j h; h.x = ws_ld2(ws, MBLS_SLOT_H, 0); h.y = ws_ld2(ws, MBLS_SLOT_H + 2, 0); h.z = ws_ld2(ws, MBLS_SLOT_H + 4, 0);
            g1j a; a.x = ws_ld(ws, MBLS_SLOT_APK, 0); a.y = ws_ld(ws, MBLS_SLOT_APK + 1, 0); a.z = ws_ld(ws, MBLS_SLOT_APK + 2, 0);
            mbls_pair pr; pr.skip = g2_is_inf(&h) | g1_is_inf(&a);
            g2h_from_jacobian(&pr.q, &h); g1arg_from_jacobian(&pr.p, &a); pr.t = pr.q;
            fp12 f; miller_loop(&f, &pr, 1);
            const fp2* c = &f.c0.c0;
            for (int s = 0; s < 6; s++) ws_st2(ws, MBLS_SLOT_F + 2 * s, 0, c[s]);
        } else
            lane_miller(ws, 0);
        for (int k = 0; k < 12; k++) fp_raw_to_be(out576 + 576 * i + 48 * k, fp_from_mont(ws_ld(ws, MBLS_SLOT_F + k, 0)));
    }
    free(ws.w);
}
// the compiled final exponentiation (lane_final's fallback body: mbls_final_exp_probe mode 0) on n elements of Fp12, 12 canonical coefficients each in the order of
// slot F: the value and fp12_is_one of it
void emul_final_exp(const uint8_t* f576, uint64_t n, uint8_t* out576, uint8_t* is_one) {
    for (uint64_t i = 0; i < n; i++) {
        fp12 f; fp* c = &f.c0.c0.c0;
        for (int k = 0; k < 12; k++) c[k] = fp_to_mont(fp_raw_from_be(f576 + 576 * i + 48 * k));
        final_exp(&f, &f);
        for (int k = 0; k < 12; k++) fp_raw_to_be(out576 + 576 * i + 48 * k, fp_from_mont(c[k]));
        is_one[i] = fp12_is_one(&f) ? 1 : 0;
    }
}
void emul_fp_mul(const uint8_t* a, const uint8_t* b, uint64_t n, uint8_t* out, int op) { for (uint64_t i = 0; i < n; i++) op_fp_mul(i, n, a, b, out, op); }
void emul_aggregate(const uint8_t* pks, int fmt, const uint32_t* offsets, uint64_t n, uint32_t k, uint8_t* out96, uint32_t* status) {
    mbls_ws ws; ws.stride = n ? n : 1; ws.w = (uint32_t*)calloc((size_t)MBLS_SLOT_COUNT * 12 * ws.stride, 4);
    const uint32_t pkb = fmt == MBLS_PK_COMPRESSED ? 48 : 96;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t first = offsets ? offsets[i] : (uint64_t)k * i; uint32_t cnt = offsets ? offsets[i + 1] - offsets[i] : k;
        lane_aggregate(ws, i, pks + pkb * first, cnt, fmt, MBLS_MODE_FAST_AGGREGATE, &status[i]);
        op_apk_export(ws, i, out96);
    }
    free(ws.w);
}
}

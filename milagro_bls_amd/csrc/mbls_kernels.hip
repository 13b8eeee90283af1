// mbls_kernels.hip -- gfx950 kernels and the C ABI of libmbls_hip.so (see include/mbls.h).
//
// One item per lane, one wave (64 lanes) per workgroup: the kernels are long integer carry-chain programs
// with no intra-workgroup cooperation, so single-wave workgroups give the dispatcher the finest granularity
// to fill 256 CUs x 4 SIMDs. The pipeline is split into phase kernels that hand their state over through a
// limb-major struct-of-arrays workspace in HBM (mbls_lanes.h); each phase is thousands of Fp
// multiplications per lane, so the hand-over traffic (<= 1.2 KB per item per phase) and the launch gaps are
// noise. No MFMA (carry-chain integer work). LDS is not used for tiling (no data is shared between lanes) but as the
// home of each lane's loop-carried state in k_miller / k_final (36 KB per wave, lane-interleaved so that a wave's access is
// conflict-free), which keeps that state out of the register file between uses and off the HBM-backed stack.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <new>
#include <mutex>
#include <vector>
#include <algorithm>
#include <atomic>
#include <dlfcn.h>
#include <unistd.h>
#include "mbls_ops.h"
#include "mbls_coop.h"
#include "mbls_vmb.h"
#include "mbls_vml.h"
#include "mbls_vms.h"
#include "mbls_vsl.h"
#include "mbls_vmt.h"
#include "mbls_mtb.h"
#include "mbls_batch.h"
#include "mbls_vmd.h"
#include "mbls_vmr.h"
#include "mbls_cmt_lanes.h"
#include "mbls_cms_launch.h"
#include "mbls_vcs_launch.h"
#include "mbls_vbg_launch.h"
#include "../../include/mbls.h"

// The product library exists only with the generated routines: the host side below selects kernels (the fused subgroup verdict of
// k_miller / k_sig_verdict, k_blind_*_d, the tree levels, k_coop) whose bodies ARE those routines. The development switches that used to
// replace them by the compiled lane bodies would leave empty or unfused kernels behind the same launches -- wrong answers, not slower
// ones -- so such a build is refused. (The compiled lane bodies remain what tests/host_emul compiles as plain C++.)
#if defined(MBLS_NO_ASM) || defined(MBLS_NO_FP2_ASM) || defined(MBLS_NO_LDS_STATE)
#error "libmbls_hip.so cannot be built with MBLS_NO_ASM / MBLS_NO_FP2_ASM / MBLS_NO_LDS_STATE: the host side depends on the generated routines"
#endif
#if defined(__HIP_DEVICE_COMPILE__) && !MBLS_DEVICE_ASM
#error "device pass without the generated routines"
#endif

// RCCL: the library is opened at run time (mbls_multi_create), never linked -- and its headers are not needed to BUILD either: the few opaque types and enumerators
// the dlopen'ed entry points take are declared here when <rccl/rccl.h> is absent (values are RCCL's / NCCL's stable ABI: ncclSuccess = 0, ncclUint8 = 1)
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
typedef struct ncclComm* ncclComm_t;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclChar = 0, ncclUint8 = 1 } ncclDataType_t;
#endif

#define MBLS_SLOT_S 25            // 6 Fp: Jacobian G2 accumulator for verify_multiple
#define MBLS_SLOT_T 31            // 12 Fp: the running points of the generated Miller loop (packed, 2^392 domain; tools/gen_tower_d.py T_SLOT)
#define MBLS_SLOT_G2TMP 43        // 6 Fp: scratch of the generated subgroup-test routine (tools/gen_tower_d.py G2_SLOTS)
#define MBLS_SLOT_KREC 49         // 60 Fp: the six compressed powers of the final exponentiation (tools/gen_tower_d.py K_SLOT, K_REC); verify_multiple's
                                  // signature phase keeps its table of 1..8 times the signature in 49..96 (BL_TAB)
#define MBLS_SLOT_G1TAB 109       // 24 Fp: verify_multiple's table of 1..8 times the aggregate key (tools/gen_tower_d.py G1B_TAB)
#define MBLS_SLOT_TOTAL 133
#define WG 64
// The pipeline kernels are built for one wave per SIMD (512 registers per lane): a batch of 2^16 items is exactly one wave
// per SIMD on 256 CUs, and the hot loops are generated straight-line routines that already issue at the VALU rate with a
// single wave, so a 256-register / two-wave variant is slower at every batch size (larger batches
// simply run as successive rounds of workgroups).
#define MBLS_LB __launch_bounds__(WG, 1)

static __device__ __forceinline__ uint64_t gid() { return (uint64_t)blockIdx.x * WG + threadIdx.x; }

// ------------------------------------------------------------------------------------------------ pipeline kernels
__global__ void MBLS_LB k_aggregate(mbls_ws ws, const uint8_t* pks, const uint32_t* offsets, uint32_t k, int fmt, int mode,
                                                   uint32_t* status, uint64_t n) {
    uint64_t i = gid(); if (i >= n) return;
    const uint32_t pkb = fmt == MBLS_PK_COMPRESSED ? 48u : 96u;
    uint64_t first = offsets ? offsets[i] : (uint64_t)k * i; uint32_t cnt = offsets ? offsets[i + 1] - offsets[i] : k;
    uint32_t bad = 0;
    if (offsets && offsets[i + 1] < offsets[i]) { cnt = 0; bad = MBLS_ST_BAD_PK_ENCODING; }     // a non-monotonic offset table never becomes a read
    uint32_t st; lane_aggregate(ws, i, pks + pkb * first, cnt, fmt, mode, &st); st |= bad; if (st) atomicOr(status + i, st);
}
// the generated routines (96-byte keys at 4-byte aligned addresses; table indices)
__global__ void MBLS_LB k_aggregate_raw_d(mbls_ws ws, const uint8_t* pks, const uint32_t* offsets, uint32_t k, int mode, uint32_t* status, uint64_t n) {
    uint64_t i = gid(); if (i >= n) return;
    uint64_t first = offsets ? offsets[i] : (uint64_t)k * i; uint32_t cnt = offsets ? offsets[i + 1] - offsets[i] : k;
    uint32_t bad = 0;
    if (offsets && offsets[i + 1] < offsets[i]) { cnt = 0; bad = MBLS_ST_BAD_PK_ENCODING; }
#if MBLS_DEVICE_ASM
    uint32_t st = lane_aggregate_d<false>(ws, i, pks + 96 * first, cnt, mode, threadIdx.x) | bad;
    if (st) atomicOr(status + i, st);
#endif
}
__global__ void MBLS_LB k_aggregate_indexed_d(mbls_ws ws, const uint32_t* recs, uint64_t tsize, const uint32_t* idx, const uint32_t* offsets, uint32_t k,
                                              int mode, uint32_t* status, uint64_t n) {
    uint64_t i = gid(); if (i >= n) return;
    uint64_t first = offsets ? offsets[i] : (uint64_t)k * i; uint32_t cnt = offsets ? offsets[i + 1] - offsets[i] : k;
    uint32_t bad = 0;
    if (offsets && offsets[i + 1] < offsets[i]) { cnt = 0; bad = MBLS_ST_BAD_PK_ENCODING; }
#if MBLS_DEVICE_ASM
    uint32_t st = lane_aggregate_d<true>(ws, i, idx + first, cnt, mode, threadIdx.x, recs, tsize) | bad;
    if (st) atomicOr(status + i, st);
#endif
}
// one key per lane, nothing but a square root: with the 8-entry window table (112 AGPRs) the kernel fits 256 registers and two
// waves share a SIMD -- the plain 32-bit third of the instruction stream then issues at twice the rate (profiles/r02_ubench.txt)
// Small batches (the wave engine's: latency): the key sum of an item is cut into MBLS_KEY_SPLIT partial sums on lanes of their own (k_aggregate_raw_d /
// k_aggregate_indexed_d over n * MBLS_KEY_SPLIT sub-items, whose keys lie back to back exactly like items of k / MBLS_KEY_SPLIT keys; their sums in the APK slots of
// workspace items n + i * MBLS_KEY_SPLIT + q, their status words in st_sub) and this kernel adds the partial sums of item i -- AggregatePublicKey::aggregate
// (reference src/aggregates.rs:29-39) sums from infinity in any order to the same point --, folds the status words and applies the apk = infinity test.
#define MBLS_KEY_SPLIT 8u
__global__ void MBLS_LB k_apk_combine(mbls_ws ws, uint64_t n, int mode, const uint32_t* st_sub, uint32_t* status) {
    uint64_t i = gid(); if (i >= n) return;
    const uint64_t t0 = n + i * MBLS_KEY_SPLIT;
    g1j acc; acc.x = ws_ld(ws, MBLS_SLOT_APK, t0); acc.y = ws_ld(ws, MBLS_SLOT_APK + 1, t0); acc.z = ws_ld(ws, MBLS_SLOT_APK + 2, t0);
    uint32_t st = st_sub[i * MBLS_KEY_SPLIT];
    for (uint32_t q = 1; q < MBLS_KEY_SPLIT; q++) {
        g1j p; p.x = ws_ld(ws, MBLS_SLOT_APK, t0 + q); p.y = ws_ld(ws, MBLS_SLOT_APK + 1, t0 + q); p.z = ws_ld(ws, MBLS_SLOT_APK + 2, t0 + q);
        g1_add(&acc, &acc, &p);
        st |= st_sub[i * MBLS_KEY_SPLIT + q];
    }
    if (mode == MBLS_MODE_FAST_AGGREGATE && g1_is_inf(&acc)) st |= MBLS_ST_APK_INFINITY;
    ws_st(ws, MBLS_SLOT_APK, i, acc.x); ws_st(ws, MBLS_SLOT_APK + 1, i, acc.y); ws_st(ws, MBLS_SLOT_APK + 2, i, acc.z);
    if (st) atomicOr(status + i, st);
}
// Committee table (include/mbls.h "committee table", mbls_cmt.h, mbls_cmt_lanes.h). k_cmt_expand: one wave per item turns (committee, bitfield) into the item's
// index list -- the selected members, or on the complement route the missing ones --, 64 members per step; k_aggregate_cmt_d is k_aggregate_indexed_d over those
// lists with the complement's fix-up addition and the status word formed from the final point; k_cmt_build makes the records of an append from the sums
// k_aggregate_indexed_d left in the workspace.
__global__ void __launch_bounds__(WG) k_cmt_expand(const uint32_t* crecs, uint64_t ccount, const uint32_t* members, const uint32_t* cmt_idx, const uint8_t* bits,
                                                   uint32_t bits_stride, int mode, uint32_t* list, uint64_t list_stride, uint32_t* cnt, uint32_t* route, uint64_t n) {
    const uint64_t i = blockIdx.x; if (i >= n) return;
    wave_cmt_expand(i, threadIdx.x, crecs, ccount, members, cmt_idx, bits, bits_stride, mode, list, list_stride, cnt, route);
}
__global__ void MBLS_LB k_aggregate_cmt_d(mbls_ws ws, const uint32_t* recs, uint64_t tsize, const uint32_t* list, uint64_t list_stride, const uint32_t* cnt,
                                          const uint32_t* route, const uint32_t* crecs, const uint32_t* cmt_idx, uint32_t* status, uint64_t n) {
    uint64_t i = gid(); if (i >= n) return;
#if MBLS_DEVICE_ASM
    uint32_t st = lane_aggregate_cmt(ws, i, threadIdx.x, recs, tsize, list, list_stride, cnt, route, crecs, cmt_idx);
    if (st) atomicOr(status + i, st);
#endif
}
// verify_multiple over committees (mbls_vmc.h): k_vmc_expand is k_cmt_expand with the single-key sets of a gossip batch beside the committee sets; k_aggregate_vmc_d
// is k_aggregate_cmt_d's body with the status word cut to what verify_multiple's key phase reports (vmc_key_status: the indexed key sum of those entries flags
// neither the empty list nor the sum at infinity). A complement set is always a committee set, so cmt_idx[i] is a committee id wherever the body reads it as one.
__global__ void __launch_bounds__(WG) k_vmc_expand(const uint32_t* crecs, uint64_t ccount, const uint32_t* members, const uint32_t* cmt_idx, const uint8_t* bits,
                                                   uint32_t bits_stride, int mode, uint32_t* list, uint64_t list_stride, uint32_t* cnt, uint32_t* route, uint64_t n) {
    const uint64_t i = blockIdx.x; if (i >= n) return;
    wave_vmc_expand(i, threadIdx.x, crecs, ccount, members, cmt_idx, bits, bits_stride, mode, list, list_stride, cnt, route);
}
__global__ void MBLS_LB k_aggregate_vmc_d(mbls_ws ws, const uint32_t* recs, uint64_t tsize, const uint32_t* list, uint64_t list_stride, const uint32_t* cnt,
                                          const uint32_t* route, const uint32_t* crecs, const uint32_t* cmt_idx, uint32_t* status, uint64_t n) {
    uint64_t i = gid(); if (i >= n) return;
#if MBLS_DEVICE_ASM
    uint32_t st = vmc_key_status(lane_aggregate_cmt(ws, i, threadIdx.x, recs, tsize, list, list_stride, cnt, route, crecs, cmt_idx));
    if (st) atomicOr(status + i, st);
#endif
}
__global__ void MBLS_LB k_cmt_build(mbls_ws ws, const uint32_t* st, const uint32_t* offsets, uint64_t member_base, uint32_t* crecs, uint64_t n) {
    uint64_t c = gid(); if (c < n) lane_cmt_build(ws, c, st, offsets, member_base, crecs);
}
__global__ void MBLS_LB k_cmt_export(const uint32_t* rec, uint8_t* out96) { if (gid() == 0) lane_cmt_export(rec, out96); }
__global__ void __launch_bounds__(WG, 2) k_pk_decompress(const uint8_t* pks48, uint64_t nkeys, uint32_t* keys_xy, uint8_t* flags) {
    uint64_t j = gid(); if (j >= nkeys) return;
    lane_pk_decompress(j, pks48, keys_xy, flags);
}
__global__ void MBLS_LB k_aggregate_decoded(mbls_ws ws, const uint32_t* keys_xy, const uint8_t* flags, uint32_t k, int mode, uint32_t* status, uint64_t n) {
    uint64_t i = gid(); if (i >= n) return;
    uint32_t st; lane_aggregate_decoded(ws, i, keys_xy + 24 * (uint64_t)k * i, flags + (uint64_t)k * i, k, mode, &st); if (st) atomicOr(status + i, st);
}
// Resident key table (the on-device analogue of the decoded PublicKey objects a reference caller holds, src/keys.rs:116-120):
// item i sums the table entries idx[k*i .. k*i+k) (or idx[offsets[i] .. offsets[i+1])).
__global__ void MBLS_LB k_aggregate_indexed(mbls_ws ws, const uint32_t* recs, uint64_t tsize, const uint32_t* idx, const uint32_t* offsets, uint32_t k,
                                            int mode, uint32_t* status, uint64_t n) {
    uint64_t i = gid(); if (i >= n) return;
    uint64_t first = offsets ? offsets[i] : (uint64_t)k * i; uint32_t cnt = offsets ? offsets[i + 1] - offsets[i] : k;
    uint32_t bad = 0;
    if (offsets && offsets[i + 1] < offsets[i]) { cnt = 0; bad = MBLS_ST_BAD_PK_ENCODING; }
    uint32_t st; lane_aggregate_indexed(ws, i, recs, tsize, idx + first, cnt, mode, &st); st |= bad; if (st) atomicOr(status + i, st);
}
// n x PublicKey::from_bytes[_unchecked] / from_uncompressed_bytes into table records (affine Montgomery limbs + flags)
__global__ void MBLS_LB k_keytable_append(const uint8_t* in, int fmt, int validate, uint64_t n, uint32_t* recs, uint8_t* errs) {
    uint64_t i = gid(); if (i < n) op_keytable_append(i, in, fmt, validate, recs, errs);
}
__global__ void MBLS_LB k_keytable_export(const uint32_t* recs, uint64_t first, uint64_t n, uint8_t* out96, uint8_t* errs) {
    uint64_t i = gid(); if (i < n) op_keytable_export(i, recs + 32 * first, out96, errs);
}
// batched AggregateSignature::aggregate (src/aggregates.rs:100-106): decode one signature per lane, then one set per lane
__global__ void MBLS_LB k_g2_decode_affine(const uint8_t* sigs96, uint64_t n, uint32_t* xy, uint8_t* flags) {
    uint64_t i = gid(); if (i < n) op_g2_decode_affine(i, sigs96, xy, flags);
}
__global__ void MBLS_LB k_g2_sum(const uint32_t* xy, const uint8_t* flags, const uint32_t* offsets, uint32_t k, uint64_t n, uint8_t* out96, uint8_t* errs) {
    uint64_t i = gid(); if (i >= n) return;
    uint64_t first = offsets ? offsets[i] : (uint64_t)k * i; uint32_t cnt = offsets ? offsets[i + 1] - offsets[i] : k;
    if (offsets && offsets[i + 1] < offsets[i]) cnt = 0;
    op_g2_sum(i, xy + 48 * first, flags + first, cnt, out96, errs);
}
__global__ void MBLS_LB k_sig(mbls_ws ws, const uint8_t* sigs, uint32_t* status, uint64_t n, int check) {
    __shared__ uint32_t spill[154 * 64];          // 11 spill slots of 14 dwords per lane for the generated subgroup test
    uint64_t i = gid(); if (i >= n) return;
    uint32_t st = 0; lane_sig(ws, i, sigs + 96 * i, &st, (MBLS_LDS uint32_t*)spill, threadIdx.x, true, check != 0);
    if (st) atomicOr(status + i, st);             // may run beside k_aggregate on another stream
}
// item i's message: msgs[mlen i ..] or, with an offset table of n + 1 entries, msgs[moff[i] .. moff[i+1]) (any length below 2^32; a range
// that runs backwards is never read: the item is rejected with MBLS_ST_BAD_MSG_RANGE)
__global__ void MBLS_LB k_hash(mbls_ws ws, const uint8_t* msgs, uint32_t mlen, const uint64_t* moff, uint32_t* status, uint64_t n) {
    __shared__ uint32_t spill[154 * 64];          // the same for the addition / cofactor-clearing routine
    uint64_t i = gid(); if (i >= n) return;
    const uint8_t* m = msgs + (uint64_t)mlen * i; uint32_t len = mlen;
    if (moff) {
        const uint64_t a = moff[i], b = moff[i + 1];
        const bool bad = b < a || b - a > 0xFFFFFFFFull;
        m = msgs + (bad ? 0 : a); len = bad ? 0u : (uint32_t)(b - a);
        if (bad) atomicOr(status + i, MBLS_ST_BAD_MSG_RANGE);
    }
    lane_hash(ws, i, m, len, (MBLS_LDS uint32_t*)spill, threadIdx.x, true);
}
// The message phase with TWO lanes per message (batches of at most half a round): lane t = 2 i + e has workspace item t of its own, runs
// hash_to_field of message i (both lanes: 19 SHA-256 compressions are 2 % of the phase) and ONE map_to_curve -- u_e --, then the even lane adds
// the neighbour's point, clears the cofactor and leaves H in item 2 i; k_h_compact_a / _b move it to item i (through slots 19..24: item i's
// slots 7..12 may still be the working slots of another pair's lane while this kernel runs).
__global__ void MBLS_LB k_hash2(mbls_ws ws, const uint8_t* msgs, uint32_t mlen, const uint64_t* moff, uint32_t* status, uint64_t n) {
    __shared__ uint32_t spill[154 * 64];
    const uint64_t t = gid(); if (t >= 2 * n) return;
    const uint64_t i = t >> 1;
    const uint8_t* m = msgs + (uint64_t)mlen * i; uint32_t len = mlen;
    if (moff) {
        const uint64_t a = moff[i], b = moff[i + 1];
        const bool bad = b < a || b - a > 0xFFFFFFFFull;
        m = msgs + (bad ? 0 : a); len = bad ? 0u : (uint32_t)(b - a);
        if (bad && !(t & 1)) atomicOr(status + i, MBLS_ST_BAD_MSG_RANGE);
    }
#if MBLS_DEVICE_ASM
    hash_fields_to_ws(ws.w, ws.stride, t, m, len, (uint32_t)(t & 1));
    g2_hash2_d_call(ws, t, (MBLS_LDS uint32_t*)spill, threadIdx.x);
#endif
}
__global__ void __launch_bounds__(WG) k_h_compact_a(mbls_ws ws, uint64_t n) {
    uint64_t i = gid(); if (i >= n) return;
    for (int w = 0; w < 72; w++) ws.w[((uint64_t)(19 * 12 + w)) * ws.stride + i] = ws.w[((uint64_t)(MBLS_SLOT_H * 12 + w)) * ws.stride + 2 * i];
}
__global__ void __launch_bounds__(WG) k_h_compact_b(mbls_ws ws, uint64_t n) {
    uint64_t i = gid(); if (i >= n) return;
    for (int w = 0; w < 72; w++) ws.w[((uint64_t)(MBLS_SLOT_H * 12 + w)) * ws.stride + i] = ws.w[((uint64_t)(19 * 12 + w)) * ws.stride + i];
}
// Shared message lists (mbls_*_shared_msgs): the points of the m messages a piece of the list hash left in slot H of workspace items [0, m) go to the context's
// table (entries first_entry + i; lane_h_export), and every item of a pass copies the entry its index names into its own slot H (lane_h_gather). Copies and
// nothing else: 72 dword loads and stores per lane, consecutive lanes = consecutive items / entries on the strided side, a few registers -- blocks of four waves,
// eight waves per SIMD, no LDS. (The gather's reads follow the indices: with a few hundred messages the table is a few tens of KB and stays in cache.)
// (k_h_export_tab: k_h_export is the hash probe's kernel further down, which writes compressed points)
#define MBLS_HB 256
__global__ void __launch_bounds__(MBLS_HB) k_h_export_tab(mbls_ws ws, uint32_t* tab, uint64_t tstride, uint32_t* flags, const uint32_t* st_list, uint64_t first_entry, uint64_t m) {
    const uint64_t i = (uint64_t)blockIdx.x * MBLS_HB + threadIdx.x; if (i >= m) return;
    lane_h_export(ws, i, tab, tstride, first_entry + i, flags, st_list);
}
__global__ void __launch_bounds__(MBLS_HB) k_h_gather(mbls_ws ws, const uint32_t* tab, uint64_t tstride, const uint32_t* flags, const uint32_t* msg_idx, uint64_t n_msgs,
                                                      uint32_t* status, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * MBLS_HB + threadIdx.x; if (i >= n) return;
    const uint32_t st = lane_h_gather(ws, i, tab, tstride, flags, msg_idx[i], n_msgs);
    if (st) atomicOr(status + i, st);             // beside the key sum and the signature phase, like k_hash
}
// Resident message table (mbls_msgtable_*, mbls_mtb.h). Growth: the stride follows the capacity, so every entry [0, entries) -- the private one included -- moves
// to its place in the new buffers, one lane per entry (consecutive lanes = consecutive entries on both sides). mbls_msgtable_get: entries first .. first + n - 1
// into slot H of workspace items [0, n) (k_h_export compresses them from there), errs[i] = MBLS_ERR_ARGUMENT for a flagged entry.
__global__ void __launch_bounds__(MBLS_HB) k_mtb_relayout(const uint32_t* old_tab, uint64_t old_stride, const uint32_t* old_flags, uint32_t* new_tab, uint64_t new_stride,
                                                          uint32_t* new_flags, uint64_t entries) {
    const uint64_t e = (uint64_t)blockIdx.x * MBLS_HB + threadIdx.x; if (e >= entries) return;
    mtb_relayout_entry(old_tab, old_stride, old_flags, new_tab, new_stride, new_flags, e);
}
__global__ void __launch_bounds__(MBLS_HB) k_mtb_get(mbls_ws ws, const uint32_t* tab, uint64_t tstride, const uint32_t* flags, uint64_t first, uint64_t size, uint8_t* errs,
                                                     uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * MBLS_HB + threadIdx.x; if (i >= n) return;
    const uint32_t st = lane_h_gather(ws, i, tab, tstride, flags, (uint32_t)(first + i), size);
    errs[i] = st ? (uint8_t)MBLS_ERR_ARGUMENT : (uint8_t)MBLS_OK;
}
// hash_to_field alone (SHA-256 / expand_message_xmd, one lane per item): u0, u1 into slots 31, 32 / 37, 38 -- the input of the cooperative
// engine's hashg2 program (small batches: one WAVE per item walks the maps, the addition and the cofactor clearing)
__global__ void MBLS_LB k_hash_fields(mbls_ws ws, const uint8_t* msgs, uint32_t mlen, const uint64_t* moff, uint32_t* status, uint64_t n) {
    uint64_t i = gid(); if (i >= n) return;
    const uint8_t* m = msgs + (uint64_t)mlen * i; uint32_t len = mlen;
    if (moff) {
        const uint64_t a = moff[i], b = moff[i + 1];
        const bool bad = b < a || b - a > 0xFFFFFFFFull;
        m = msgs + (bad ? 0 : a); len = bad ? 0u : (uint32_t)(b - a);
        if (bad) atomicOr(status + i, MBLS_ST_BAD_MSG_RANGE);
    }
#if MBLS_DEVICE_ASM
    hash_fields_to_ws(ws.w, ws.stride, i, m, len);
#endif
}
// Test probe (mbls_map_to_g2_probe): the message phase AFTER hash_to_field on field elements the caller names -- the branches no hashed message reaches (u = 0,
// sgn0 with a zero real part, q0 = +-q1). k_map_import stands in for hash_fields_to_ws: item i's four values (canonical 48-byte big-endian) in Montgomery form
// into slots 31, 32 / 37, 38; pair != 0: two lanes per message, lane t = 2 i + e stores into ITS item t, the odd lane with u0 and u1 exchanged (k_hash2's swap).
// k_map_lane / k_map_pair are k_hash / k_hash2 from that point on: the same launch shape, the same LDS array, the same generated routines.
__global__ void __launch_bounds__(WG) k_map_import(mbls_ws ws, const uint8_t* u192, uint64_t n, int pair) {
    const uint64_t t = gid(); if (t >= (pair ? 2 * n : n)) return;
    const uint64_t i = pair ? t >> 1 : t; const uint32_t swap = pair ? (uint32_t)(t & 1) : 0u;
    for (uint32_t k = 0; k < 4; k++)
        ws_st(ws, (int)(31 + (k & 1) + 6 * ((k >> 1) ^ swap)), t, fp_to_mont(fp_raw_from_be(u192 + 192 * i + 48 * k)));
}
__global__ void MBLS_LB k_map_lane(mbls_ws ws, uint64_t n) {
#if MBLS_DEVICE_ASM
    __shared__ uint32_t spill[154 * 64];
    uint64_t i = gid(); if (i >= n) return;
    g2_group_d_call<true>(ws, i, (MBLS_LDS uint32_t*)spill, threadIdx.x);
#endif
}
__global__ void MBLS_LB k_map_pair(mbls_ws ws, uint64_t n) {
#if MBLS_DEVICE_ASM
    __shared__ uint32_t spill[154 * 64];
    const uint64_t t = gid(); if (t >= 2 * n) return;
    g2_hash2_d_call(ws, t, (MBLS_LDS uint32_t*)spill, threadIdx.x);
#endif
}
// the compiled body of the same steps (mbls_hash.h / mbls_curve.h)
__global__ void MBLS_LB k_map_body(mbls_ws ws, uint64_t n) {
    uint64_t i = gid(); if (i >= n) return;
    const fp2 u0 = ws_ld2(ws, 31, i), u1 = ws_ld2(ws, 37, i);
    g2j q0, q1, h; map_to_curve_g2(&q0, &u0); map_to_curve_g2(&q1, &u1);
    g2_add(&q0, &q0, &q1); g2_clear_cofactor(&h, &q0);
    ws_st2(ws, MBLS_SLOT_H, i, h.x); ws_st2(ws, MBLS_SLOT_H + 2, i, h.y); ws_st2(ws, MBLS_SLOT_H + 4, i, h.z);
}
__global__ void MBLS_LB k_miller(mbls_ws ws, uint64_t n) {
    // one wave per SIMD = 4 waves per CU: each wave can park 36 KB of loop state in LDS (144 of the 160 KB)
    __shared__ uint32_t tstore[154 * 64];         // 11 spill slots of 14 dwords per lane for the generated loop (the running points are in HBM)
    uint64_t i = gid(); if (i >= n) return;
    lane_miller(ws, i, (MBLS_LDS uint32_t*)tstore, threadIdx.x, true);
}
// between k_miller and k_final when k_sig only decoded: the signature's subgroup test from the loop's running point (lane_sig_verdict)
__global__ void MBLS_LB k_sig_verdict(mbls_ws ws, uint32_t* status, uint64_t n, uint64_t t_item_offset, int t_pair) {
    uint64_t i = gid(); if (i >= n) return;
    const uint32_t st = lane_sig_verdict(ws, i, i + t_item_offset, t_pair);
    if (st) status[i] |= st;
}
// Batches that fill at most half of the SIMDs (2 n <= one round): the two pairs of item i on TWO lanes -- lane i walks (H_i, apk_i), lane n + i
// walks (sig_i, -G1) -- each with the generated one-pair loop (6.6 ms instead of 11.3 for the two-pair loop), workspace item = lane. The
// product f_i f_(n+i) is one level of the generated product tree (k_f12_tree_d(2 n, n)), and the signature's subgroup verdict reads the running
// point of lane n + i (k_sig_verdict with t_item_offset = n, t_pair = 1): the one-pair routine walks the same bits of |x| with the same
// incomplete formulas (Q in homogeneous form with Z = 1), so it ends with [|x|] sig exactly like pair 0 of the two-pair loop.
// lpp = 2 (batches of at most a quarter of a round): TWO lanes per pair -- lanes 2 q, 2 q + 1 walk pair q together, their products in pairs
// (miller_loop_single_pair_d): four lanes per item.
template <int LPP> MBLS_FN void miller_split_body(const mbls_ws& ws, uint64_t n, uint32_t* spill) {
    const uint64_t lane_id = gid();
    uint64_t t = LPP == 2 ? lane_id >> 1 : lane_id; if (t >= 2 * n) return;
    const bool sigpair = t >= n;                                   // branch-free operand selection: the routine is called from uniform control flow
    const uint64_t i = sigpair ? t - n : t;
    g2j h; h.x = ws_ld2(ws, MBLS_SLOT_H, i); h.y = ws_ld2(ws, MBLS_SLOT_H + 2, i); h.z = ws_ld2(ws, MBLS_SLOT_H + 4, i);
    g1j a; a.x = ws_ld(ws, MBLS_SLOT_APK, i); a.y = ws_ld(ws, MBLS_SLOT_APK + 1, i); a.z = ws_ld(ws, MBLS_SLOT_APK + 2, i);
    const fp2 sx = ws_ld2(ws, MBLS_SLOT_SIG, i), sy = ws_ld2(ws, MBLS_SLOT_SIG + 2, i);
    mbls_pair pr, ps;
    pr.skip = g2_is_inf(&h) | g1_is_inf(&a);
    g2h_from_jacobian(&pr.q, &h); g1arg_from_jacobian(&pr.p, &a);
    ps.skip = fp2_is_zero(sy);
    g2h_from_affine(&ps.q, sx, sy); g1arg_from_affine(&ps.p, fp_load_const(MBLS_G1_X), fp_load_const(MBLS_G1_NEG_Y));
    pr.skip = sigpair ? ps.skip : pr.skip;
    pr.q.x = fp2_select(sigpair, ps.q.x, pr.q.x); pr.q.y = fp2_select(sigpair, ps.q.y, pr.q.y); pr.q.z = fp2_select(sigpair, ps.q.z, pr.q.z);
    pr.p.px = fp_select(sigpair, ps.p.px, pr.p.px); pr.p.py = fp_select(sigpair, ps.p.py, pr.p.py); pr.p.pz3 = fp_select(sigpair, ps.p.pz3, pr.p.pz3);
    pr.t = pr.q;
    fp12 f;
#if MBLS_DEVICE_ASM
    if (LPP == 2) miller_loop_single_pair_d(&f, &pr, ws.w, ws.stride, t, (MBLS_LDS uint32_t*)spill, threadIdx.x);
    else miller_loop_single_d(&f, &pr, ws.w, ws.stride, t, (MBLS_LDS uint32_t*)spill, threadIdx.x);
#endif
    const fp2* c = &f.c0.c0;
    for (int s = 0; s < 6; s++) ws_st2(ws, MBLS_SLOT_F + 2 * s, t, c[s]);
}
__global__ void MBLS_LB k_miller_split(mbls_ws ws, uint64_t n) {
    __shared__ uint32_t spill[154 * 64];
    miller_split_body<1>(ws, n, spill);
}
__global__ void MBLS_LB k_miller_split4(mbls_ws ws, uint64_t n) {      // four lanes per item: two per pair
    __shared__ uint32_t spill[154 * 64];
    miller_split_body<2>(ws, n, spill);
}
__global__ void MBLS_LB k_final(mbls_ws ws, uint32_t* status, uint8_t* results, uint64_t n) {
    __shared__ uint32_t accstore[154 * 64];       // spill slots of the generated exponentiation routine / the Fp12 parked by the one-shot products
    uint64_t i = gid(); if (i >= n) return;
    uint32_t st = status[i]; uint8_t r; lane_final(ws, i, &st, &r, (MBLS_LDS uint32_t*)accstore, threadIdx.x, true); status[i] = st; results[i] = r;
}

// The final exponentiation with TWO lanes per item (batches of at most half a round: the SIMDs a one-lane launch would leave idle do half of
// every compressed squaring): lanes 2 j, 2 j + 1 of a workgroup = item 32 blockIdx + j. Both lanes end with the same value; the even one reports.
__global__ void MBLS_LB k_final2(mbls_ws ws, uint32_t* status, uint8_t* results, uint64_t n) {
    __shared__ uint32_t accstore[154 * 64];       // one column per ITEM: the two lanes of an item park identical values in it
    const uint64_t t = gid(); if (t >= 2 * n) return;
    const uint64_t i = t >> 1;
#if MBLS_DEVICE_ASM
    uint32_t st = status[i]; uint8_t r;
    lane_final2(ws, i, &st, &r, (MBLS_LDS uint32_t*)accstore, threadIdx.x);
    if ((t & 1) == 0) { status[i] = st; results[i] = r; }
#endif
}

// accept bitmap: one 64-bit word per wave via ballot
__global__ void MBLS_LB k_pack(const uint8_t* results, uint64_t* bitmap, uint64_t n) {
    uint64_t i = gid();
    bool bit = (i < n) && results[i];
    uint64_t m = __ballot(bit);
    if (threadIdx.x == 0) bitmap[blockIdx.x] = m;
}

// ------------------------------------------------------------------------------------------------ n-pairing kernels
// (aggregate_verify, reference src/aggregates.rs:130-170; verify_multiple, src/aggregates.rs:261-316)
// item i: f_i = Miller(H_i, P_i) with P_i = [r_i] pk_i (r_i = 1 when rands == NULL: aggregate_verify only); S_i = [r_i] sig_i.
// The G1 and the G2 halves are kernels of their own so that they can run side by side on two streams (sets below 2^14 leave most SIMDs
// idle); both OR their bits into status[i] atomically. A zero scalar would drop set i from the check: it is flagged, never used.
// k_blind_g1 (compiled) serves aggregate_verify (rands == NULL: no multiplication); verify_multiple runs the generated k_blind_*_d.
__global__ void MBLS_LB k_blind_g1(mbls_ws ws, const uint8_t* pks96, const uint64_t* rands, uint32_t* status, uint64_t n) {
    uint64_t i = gid(); if (i >= n) return;
    uint32_t st = 0;
    g1j p;
    if (pks96) {
        fp x, y; bool inf; int e = g1_decode_uncompressed(&x, &y, &inf, pks96 + 96 * i);
        if (e) { st |= MBLS_ST_BAD_PK_ENCODING; inf = true; }
        p.x = x; p.y = y; p.z = fp_one(); if (inf) g1_set_inf(&p);
    } else {          // aggregate key left in the workspace by k_aggregate (which already set the status bits)
        p.x = ws_ld(ws, MBLS_SLOT_APK, i); p.y = ws_ld(ws, MBLS_SLOT_APK + 1, i); p.z = ws_ld(ws, MBLS_SLOT_APK + 2, i);
    }
    if (rands) {
        uint32_t k[2] = {(uint32_t)rands[i], (uint32_t)(rands[i] >> 32)};
        if ((k[0] | k[1]) == 0) st |= MBLS_ST_BAD_SCALAR;
        g1_mul(&p, &p, k, 64);
    }
    ws_st(ws, MBLS_SLOT_APK, i, p.x); ws_st(ws, MBLS_SLOT_APK + 1, i, p.y); ws_st(ws, MBLS_SLOT_APK + 2, i, p.z);
    if (st) atomicOr(status + i, st);
}
// [r_i] pk_i with the generated windowed routine (g1_blind_routine); pks96 == NULL: the aggregate key k_aggregate left in slots 0..2
__global__ void MBLS_LB k_blind_g1_d(mbls_ws ws, const uint8_t* pks96, const uint64_t* rands, uint32_t* status, uint64_t n) {
#if MBLS_DEVICE_ASM
    uint64_t i = gid(); if (i >= n) return;
    uint32_t st = 0;
    if (pks96) {
        fp x, y; bool inf; int e = g1_decode_uncompressed(&x, &y, &inf, pks96 + 96 * i);
        if (e) { st |= MBLS_ST_BAD_PK_ENCODING; inf = true; }
        g1j p; p.x = x; p.y = y; p.z = fp_one(); if (inf) g1_set_inf(&p);
        ws_st(ws, MBLS_SLOT_APK, i, p.x); ws_st(ws, MBLS_SLOT_APK + 1, i, p.y); ws_st(ws, MBLS_SLOT_APK + 2, i, p.z);
    }
    const uint64_t r = rands[i];
    if (r == 0) st |= MBLS_ST_BAD_SCALAR;
    g1_blind_d_call(ws, i, threadIdx.x, r);
    if (st) atomicOr(status + i, st);
#endif
}
// the same with the generated routines (decode inlined like k_sig; subgroup test + windowed [r] sig: g2_blind_routine): no lane-private memory
__global__ void MBLS_LB k_blind_sig_d(mbls_ws ws, const uint8_t* sigs96, const uint64_t* rands, uint32_t* status, uint64_t n) {
#if MBLS_DEVICE_ASM
    __shared__ uint32_t spill[154 * 64];
    uint64_t i = gid(); if (i >= n) return;
    uint32_t st = 0;
    bool inf;
    if (sigs96) {
        fp2 x, y;
        int e = g2_decode_compressed_t<true>(&x, &y, &inf, sigs96 + 96 * i);
        if (e) { st |= MBLS_ST_BAD_SIG_ENCODING; inf = true; }
        if (inf) { x = fp2_zero(); y = fp2_zero(); }
        ws_st2(ws, MBLS_SLOT_SIG, i, x); ws_st2(ws, MBLS_SLOT_SIG + 2, i, y);
    } else      // sigs96 == NULL: k_sig decoded AND tested the signatures already (they are in the slots; y = 0: infinity): only [r] sig is left to do
        inf = fp2_is_zero(ws_ld2(ws, MBLS_SLOT_SIG + 2, i));
    const uint64_t r = rands[i];
    if (r == 0) st |= MBLS_ST_BAD_SCALAR;
    // an infinite (or undecodable) signature is (0, 0) in the slots: with the scalar 0 every window digit is 0 and the sum stays at infinity
    const uint32_t fl = g2_blind_d_call(ws, i, (MBLS_LDS uint32_t*)spill, threadIdx.x, inf ? 0 : r, sigs96 ? 0u : 1u);
    if (!((fl & 1u) | inf)) st |= MBLS_ST_SIG_NOT_IN_G2;
    if (st) atomicOr(status + i, st);
#endif
}
// The signature chain of SMALL verify_multiple batches (their Miller loops run on waves: the signatures are the critical path) with TWO lanes per signature:
// lanes 2 j, 2 j + 1 of a workgroup = item 32 blockIdx + j; both decode, both walk the generated routine on identical values, products in pairs.
// k_sig2 = k_sig with the subgroup test (the one-call entry's first phase); k_blind_sig2_d = k_blind_sig_d.
__global__ void MBLS_LB k_sig2(mbls_ws ws, const uint8_t* sigs96, uint32_t* status, uint64_t n) {
#if MBLS_DEVICE_ASM
    __shared__ uint32_t spill[154 * 64];          // one column per ITEM: the two lanes of an item park identical values in it
    const uint64_t t = gid(); if (t >= 2 * n) return;
    const uint64_t i = t >> 1;
    uint32_t st = 0;
    fp2 x, y; bool inf;
    int e = g2_decode_compressed_t<true>(&x, &y, &inf, sigs96 + 96 * i);
    if (e) { st |= MBLS_ST_BAD_SIG_ENCODING; inf = true; }
    if (inf) { x = fp2_zero(); y = fp2_zero(); }
    ws_st2(ws, MBLS_SLOT_SIG, i, x); ws_st2(ws, MBLS_SLOT_SIG + 2, i, y);
    const uint32_t fl = g2_subgroup2_d_call(ws, i, (MBLS_LDS uint32_t*)spill, threadIdx.x);
    if (!((fl & 1u) | inf)) st |= MBLS_ST_SIG_NOT_IN_G2;
    if (st && !(t & 1)) atomicOr(status + i, st);
#endif
}
__global__ void MBLS_LB k_blind_sig2_d(mbls_ws ws, const uint8_t* sigs96, const uint64_t* rands, uint32_t* status, uint64_t n) {
#if MBLS_DEVICE_ASM
    __shared__ uint32_t spill[154 * 64];
    const uint64_t t = gid(); if (t >= 2 * n) return;
    const uint64_t i = t >> 1;
    uint32_t st = 0;
    bool inf;
    if (sigs96) {
        fp2 x, y;
        int e = g2_decode_compressed_t<true>(&x, &y, &inf, sigs96 + 96 * i);
        if (e) { st |= MBLS_ST_BAD_SIG_ENCODING; inf = true; }
        if (inf) { x = fp2_zero(); y = fp2_zero(); }
        ws_st2(ws, MBLS_SLOT_SIG, i, x); ws_st2(ws, MBLS_SLOT_SIG + 2, i, y);
    } else
        inf = fp2_is_zero(ws_ld2(ws, MBLS_SLOT_SIG + 2, i));
    const uint64_t r = rands[i];
    if (r == 0) st |= MBLS_ST_BAD_SCALAR;
    const uint32_t fl = g2_blind2_d_call(ws, i, (MBLS_LDS uint32_t*)spill, threadIdx.x, inf ? 0 : r, sigs96 ? 0u : 1u);
    if (!((fl & 1u) | inf)) st |= MBLS_ST_SIG_NOT_IN_G2;
    if (st && !(t & 1)) atomicOr(status + i, st);
#endif
}
// f_i = Miller(H_i, P_i) for i < n; lane n (if with_sig) computes Miller(S, -G1) with S read from slot S of item `s_item`.
// The loop itself is the generated single-pair routine (mbls_pairing.h, miller_loop_single_d).
template <int LPP> MBLS_FN void miller_single_body(const mbls_ws& ws, uint64_t n, int with_sig, uint64_t s_item, uint32_t* spill) {
    uint64_t i = LPP == 2 ? gid() >> 1 : gid(); if (i > n || (i == n && !with_sig)) return;
    // branch-free operand selection (lane n takes S and the constant -G1): the generated routine is called from uniform control flow
    const bool last = (i == n);
    const int qslot = last ? MBLS_SLOT_S : MBLS_SLOT_H;
    const uint64_t qitem = last ? s_item : i;
    g2j h; h.x = ws_ld2(ws, qslot, qitem); h.y = ws_ld2(ws, qslot + 2, qitem); h.z = ws_ld2(ws, qslot + 4, qitem);
    g1j a; a.x = ws_ld(ws, MBLS_SLOT_APK, i); a.y = ws_ld(ws, MBLS_SLOT_APK + 1, i); a.z = ws_ld(ws, MBLS_SLOT_APK + 2, i);
    a.x = fp_select(last, fp_load_const(MBLS_G1_X), a.x); a.y = fp_select(last, fp_load_const(MBLS_G1_NEG_Y), a.y); a.z = fp_select(last, fp_one(), a.z);
    mbls_pair pr;
    pr.skip = g2_is_inf(&h) | g1_is_inf(&a);
    g2h_from_jacobian(&pr.q, &h); g1arg_from_jacobian(&pr.p, &a);
    pr.t = pr.q;
    fp12 f;
#if MBLS_DEVICE_ASM
    if (LPP == 2) miller_loop_single_pair_d(&f, &pr, ws.w, ws.stride, i, (MBLS_LDS uint32_t*)spill, threadIdx.x);
    else miller_loop_single_d(&f, &pr, ws.w, ws.stride, i, (MBLS_LDS uint32_t*)spill, threadIdx.x);
#else
    miller_loop(&f, &pr, 1);
#endif
    const fp2* c = &f.c0.c0;
    for (int s = 0; s < 6; s++) ws_st2(ws, MBLS_SLOT_F + 2 * s, i, c[s]);
}
__global__ void MBLS_LB k_miller_single(mbls_ws ws, uint64_t n, int with_sig, uint64_t s_item) {
    __shared__ uint32_t spill[154 * 64];
    miller_single_body<1>(ws, n, with_sig, s_item, spill);
}
// two lanes per Miller loop (half a round of pairs or less): lanes 2 i, 2 i + 1 walk pair i together, their products in pairs
__global__ void MBLS_LB k_miller_single2(mbls_ws ws, uint64_t n, int with_sig, uint64_t s_item) {
    __shared__ uint32_t spill[154 * 64];
    miller_single_body<2>(ws, n, with_sig, s_item, spill);
}
// tree levels with one lane per product: item i <- item i (op) item i + half, for i + half < m (generated routines, tools/gen_tower_d.py)
__global__ void MBLS_LB k_f12_tree_d(mbls_ws ws, uint64_t m, uint64_t half) {
#if MBLS_DEVICE_ASM
    __shared__ uint32_t spill[154 * 64];
    uint64_t i = gid(); if (i + half >= m || i >= half) return;
    tree_level_d_call<false>(ws, i, half, (MBLS_LDS uint32_t*)spill, threadIdx.x);
#endif
}
__global__ void MBLS_LB k_g2_tree_d(mbls_ws ws, uint64_t m, uint64_t half) {
#if MBLS_DEVICE_ASM
    __shared__ uint32_t spill[154 * 64];
    uint64_t i = gid(); if (i + half >= m || i >= half) return;
    tree_level_d_call<true>(ws, i, half, (MBLS_LDS uint32_t*)spill, threadIdx.x);
#endif
}
// ---- batched AggregateVerify (reference src/aggregates.rs:130-170, n calls at once). Workspace items: [0, n) the (sig_i, -G1) pairs,
// [n, n + T) the T (message, key) pairs of all items back to back (item i owns pairs [off[i], off[i+1]) or k each), [n + T, 2 n + T) staging.
// item i's signature (slots SIG of item i, written by k_sig: affine, y = 0 = infinity) -> the operands of its (sig, -G1) pair in the slots
// k_miller_single reads: H = the signature (Jacobian), APK = -G1
__global__ void MBLS_LB k_sigpair_setup(mbls_ws ws, uint64_t n) {
    uint64_t i = gid(); if (i >= n) return;
    g2j s; s.x = ws_ld2(ws, MBLS_SLOT_SIG, i); s.y = ws_ld2(ws, MBLS_SLOT_SIG + 2, i); s.z = fp2_one();
    if (fp2_is_zero(s.y)) g2_set_inf(&s);
    ws_st2(ws, MBLS_SLOT_H, i, s.x); ws_st2(ws, MBLS_SLOT_H + 2, i, s.y); ws_st2(ws, MBLS_SLOT_H + 4, i, s.z);
    ws_st(ws, MBLS_SLOT_APK, i, fp_load_const(MBLS_G1_X)); ws_st(ws, MBLS_SLOT_APK + 1, i, fp_load_const(MBLS_G1_NEG_Y)); ws_st(ws, MBLS_SLOT_APK + 2, i, fp_one());
}
// pair j -> the item that owns it (ragged layouts; one lane per item walks its range)
__global__ void MBLS_LB k_pair_item_map(const uint32_t* off, uint64_t n, uint64_t total, uint32_t* map) {
    uint64_t i = gid(); if (i >= n) return;
    const uint64_t a = off[i], b = off[i + 1];
    if (b < a || b > total) return;
    for (uint64_t j = a; j < b; j++) map[j] = (uint32_t)i;
}
// one level of the per-item product trees over the pairs' Miller values: pair j (workspace item j of the view `wp`) takes its partner j + half
// when both lie in the same item's range and j is a multiple of 2 half from the start of that range. The generated tree routine, called with
// the lanes of the wave that have no product this level switched off.
__global__ void MBLS_LB k_f12_seg_tree_d(mbls_ws wp, const uint32_t* map, const uint32_t* off, uint32_t k, uint64_t n, uint64_t total, uint64_t half) {
#if MBLS_DEVICE_ASM
    __shared__ uint32_t spill[154 * 64];
    uint64_t j = gid(); if (j >= total) return;
    uint64_t lo, hi;
    if (off) {
        // map[j] = 0xFFFFFFFF: no item owns pair j (a table that does not start at 0, ends below total or runs backwards) -- never an index
        const uint32_t i = map[j]; if (i >= n) return;
        lo = off[i]; hi = off[i + 1];
        if (!(lo <= j && j < hi && hi <= total)) return;
    } else { lo = (j / k) * k; hi = lo + k; }
    const uint64_t r = j - lo;
    if (r % (2 * half) != 0 || j + half >= hi) return;
    tree_level_d_call<false>(wp, j, half, (MBLS_LDS uint32_t*)spill, threadIdx.x);
#endif
}
// item i: the product of its pairs (left in the first pair of its range by the tree) -> the staging item n + T + i (1 for an empty range);
// and the item's status = its signature's | the OR of its pairs' | MBLS_ST_NO_KEYS for an empty range (src/aggregates.rs:131-133)
__global__ void MBLS_LB k_f12_seg_gather(mbls_ws ws, const uint32_t* off, const uint32_t* map, uint32_t k, uint64_t n, uint64_t total, uint32_t* st_item, const uint32_t* st_pair) {
    uint64_t i = gid(); if (i >= n) return;
    uint64_t lo = off ? off[i] : (uint64_t)k * i, hi = off ? off[i + 1] : lo + k;
    uint32_t st = 0;
    if (hi < lo || hi > total) { st |= MBLS_ST_BAD_PK_ENCODING; hi = lo; }        // an offset table that runs backwards never becomes a read
    if (hi == lo) st |= MBLS_ST_NO_KEYS;
    // a pair of this range that another item claims as well (ranges overlap where a table ran backwards): that item's tree may have raced with this one's,
    // so the item is rejected -- an item that is NOT flagged owned every one of its pairs alone
    for (uint64_t j = lo; j < hi; j++) { st |= st_pair[j]; if (map && map[j] != (uint32_t)i) st |= MBLS_ST_BAD_PK_ENCODING; }
    fp12 f; fp12_set_one(&f);
    const fp* one = &f.c0.c0.c0;
    for (int t = 0; t < 12; t++) ws_st(ws, MBLS_SLOT_F + t, n + total + i, hi > lo ? ws_ld(ws, MBLS_SLOT_F + t, n + lo) : one[t]);
    if (st) atomicOr(st_item + i, st);
}
__global__ void MBLS_LB k_status_or(const uint32_t* status, uint64_t n, uint32_t* out) {
    uint64_t i = gid(); uint32_t v = (i < n) ? status[i] : 0;
    if (__ballot(v != 0)) { if (v) atomicOr(out, v); }
}
// ---- many verify_multiple batches in one call (mbls_verify_multiple_batches*; reference src/aggregates.rs:261-316, B calls at once). Workspace items: [0, n)
// the sets of all batches back to back (batch b owns [off[b], off[b+1]) or k each), [n, n + B) the (S_b, -G1) pairs, [n + B, n + 2 B) staging. The segment rules
// -- who takes which partner, who owns what, what a faulty table turns into -- are mbls_vmb.h's (host-testable).
// set j -> the batch that owns it (ragged layouts; one lane per batch claims the sets of its range, a faulty range claims nothing: vmb_range, vmb_claim)
__global__ void MBLS_LB k_vmb_set_map(const uint32_t* off, uint64_t B, uint64_t n, uint32_t* map) {
    const uint64_t b = gid(); if (b >= B) return;
    uint64_t lo, hi;
    if (!vmb_range(off, 0, n, b, &lo, &hi)) return;
    for (uint64_t j = lo; j < hi; j++) {
        const uint32_t found = atomicCAS(map + j, MBLS_VMB_NO_OWNER, (uint32_t)b);
        if (found != MBLS_VMB_NO_OWNER) atomicExch(map + j, vmb_claim(found, (uint32_t)b));
    }
}
// One level of the per-batch sums of the blinded signatures (slot S): the twin of k_f12_seg_tree_d on the generated G2 addition; lanes without a partner at this
// level return before the routine.
__global__ void MBLS_LB k_g2_seg_tree_d(mbls_ws ws, const uint32_t* map, const uint32_t* off, uint32_t k, uint64_t B, uint64_t n, uint64_t half) {
#if MBLS_DEVICE_ASM
    __shared__ uint32_t spill[154 * 64];
    const uint64_t j = gid();
    uint64_t lo, hi;
    if (!vmb_owner_range(map, off, k, B, n, j, &lo, &hi)) return;
    if (!vmb_takes_partner(j, lo, hi, half)) return;
    tree_level_d_call<true>(ws, j, half, (MBLS_LDS uint32_t*)spill, threadIdx.x);
#endif
}
// batch b's sum S_b (slot S at the head of its range; infinity for an empty or faulty range) -> the operands of its (S_b, -G1) pair in the slots the one-pair
// Miller kernels read, item n + b: H = S_b (Jacobian), APK = -G1 -- so that the B signature pairs ride the sets' Miller launch (k_sigpair_setup's role)
__global__ void MBLS_LB k_vmb_sigpair_setup(mbls_ws ws, const uint32_t* off, uint32_t k, uint64_t B, uint64_t n) {
    const uint64_t b = gid(); if (b >= B) return;
    uint64_t lo, hi; (void)vmb_range(off, k, n, b, &lo, &hi);
    const bool some = hi > lo;
    const uint64_t it = some ? lo : 0;                            // (item 0 exists in every workspace: an empty range reads it and keeps nothing)
    g2j o; g2_set_inf(&o);
    g2j s; s.x = ws_ld2(ws, MBLS_SLOT_S, it); s.y = ws_ld2(ws, MBLS_SLOT_S + 2, it); s.z = ws_ld2(ws, MBLS_SLOT_S + 4, it);
    s.x = fp2_select(some, s.x, o.x); s.y = fp2_select(some, s.y, o.y); s.z = fp2_select(some, s.z, o.z);
    ws_st2(ws, MBLS_SLOT_H, n + b, s.x); ws_st2(ws, MBLS_SLOT_H + 2, n + b, s.y); ws_st2(ws, MBLS_SLOT_H + 4, n + b, s.z);
    ws_st(ws, MBLS_SLOT_APK, n + b, fp_load_const(MBLS_G1_X)); ws_st(ws, MBLS_SLOT_APK + 1, n + b, fp_load_const(MBLS_G1_NEG_Y)); ws_st(ws, MBLS_SLOT_APK + 2, n + b, fp_one());
}
// the per-batch status fold, one lane per SET: set j's word is ORed into its owner's, and (ragged layouts) the owner counts the sets it owns by the map
__global__ void MBLS_LB k_vmb_status_fold(const uint32_t* map, const uint32_t* off, uint32_t k, uint64_t B, uint64_t n, const uint32_t* st_set, uint32_t* st_batch, uint32_t* owned) {
    const uint64_t j = gid();
    uint64_t lo, hi;
    if (!vmb_owner_range(map, off, k, B, n, j, &lo, &hi)) return;
    const uint64_t b = off ? map[j] : j / k;
    if (off) atomicAdd(owned + b, 1u);
    const uint32_t st = st_set[j];
    if (st) atomicOr(st_batch + b, st);
}
// the gather multiplies nothing, it collects: batch b's product from the head of its range -> staging item n + B + b (1 for an empty range), and the ownership
// verdict: a faulty range, or a range of which another batch owns a set (vmb_owns_all), rejects the batch (MBLS_ST_BAD_PK_ENCODING, as k_f12_seg_gather)
__global__ void MBLS_LB k_vmb_gather(mbls_ws ws, const uint32_t* off, uint32_t k, uint64_t B, uint64_t n, uint32_t* st_batch, const uint32_t* owned) {
    const uint64_t b = gid(); if (b >= B) return;
    uint64_t lo, hi;
    uint32_t st = 0;
    if (!vmb_range(off, k, n, b, &lo, &hi)) st |= MBLS_ST_BAD_PK_ENCODING;
    if (!vmb_owns_all(off ? owned : nullptr, b, lo, hi)) st |= MBLS_ST_BAD_PK_ENCODING;
    fp12 f; fp12_set_one(&f);
    const fp* one = &f.c0.c0.c0;
    const bool some = hi > lo;
    for (int t = 0; t < 12; t++) ws_st(ws, MBLS_SLOT_F + t, n + B + b, some ? ws_ld(ws, MBLS_SLOT_F + t, lo) : one[t]);
    if (st) atomicOr(st_batch + b, st);
}
// ---- verify_multiple over a shared message list, one Miller loop per MESSAGE (mbls_verify_multiple*_shared_msgs): prod_i e([r_i] apk_i, H(m_i)) =
// prod_j e(sum_{i: msg(i) = j} [r_i] apk_i, H(m_j)). The blinded keys (slot APK of the sets [0, n), the Jacobian form k_blind_g1_d leaves) are moved to
// POSITIONS -- workspace items pbase + p, the sets of one message next to each other --, summed there by per-message trees and the sums handed to the Miller
// items [0, miller_items). The arithmetic of groups, positions and ranges is mbls_vms.h's (host-testable). All of it is enqueued: the host never sees the indices.
// sets per message (one lane per set); a set whose index names no message joins no group and carries the bit that rejects the check
__global__ void MBLS_LB k_vms_count(const uint32_t* msg_idx, uint64_t n_msgs, uint64_t n, uint32_t* cnt, uint32_t* status) {
    const uint64_t i = gid(); if (i >= n) return;
    const uint32_t g = vms_group(msg_idx[i], n_msgs);
    if (g == MBLS_VMS_NO_GROUP) atomicOr(status + i, MBLS_ST_BAD_MSG_RANGE);
    else atomicAdd(cnt + g, 1u);
}
// off[0 .. n_msgs] = the exclusive scan of the counts: ONE workgroup, lane t sums its chunk (vms_scan_chunk), the chunk sums are scanned in LDS, lane t writes its chunk
__global__ void __launch_bounds__(MBLS_VMS_SCAN_LANES) k_vms_scan(const uint32_t* cnt, uint64_t n_msgs, uint32_t* off) {
    __shared__ uint32_t part[MBLS_VMS_SCAN_LANES];
    const uint32_t t = threadIdx.x;
    uint64_t lo, hi; vms_scan_chunk(n_msgs, MBLS_VMS_SCAN_LANES, t, &lo, &hi);
    uint32_t sum = 0;
    for (uint64_t j = lo; j < hi; j++) sum += cnt[j];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < MBLS_VMS_SCAN_LANES; d *= 2) {
        const uint32_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
    for (uint64_t j = lo; j < hi; j++) { off[j] = run; run += cnt[j]; }
    if (t == MBLS_VMS_SCAN_LANES - 1) off[n_msgs] = part[t];
}
// set i takes a position inside its message's range (vms_position; the ticket from the group's atomic counter), its blinded key moves there, and the map says
// which message the position belongs to. The order inside a group depends on the order the atomics arrive in and differs from run to run; the RESULT and the
// STATUS do not: a group's sum is a sum in the abelian group E(Fp), which g1_tree_routine computes exactly whatever the operands are (equal, opposite,
// infinite: settled by selection), so every order gives the same POINT -- in another Jacobian representation at most, and the Miller loop reads the point
// through its affine coordinates --, and the status bits are ORs over the sets.
__global__ void MBLS_LB k_vms_scatter(mbls_ws ws, const uint32_t* msg_idx, uint64_t n_msgs, uint64_t n, const uint32_t* off, uint32_t* cur, uint32_t* map, uint64_t pbase) {
    const uint64_t i = gid(); if (i >= n) return;
    const uint32_t g = vms_group(msg_idx[i], n_msgs);
    if (g == MBLS_VMS_NO_GROUP) return;
    const uint64_t p = vms_position(off, g, atomicAdd(cur + g, 1u));
    if (p >= n) return;                                                // (tickets stay below the count: the counts were taken from the same indices)
    map[p] = g;
    const uint32_t* src = ws.w + (uint64_t)MBLS_SLOT_APK * 12 * ws.stride + i;
    uint32_t* dst = ws.w + (uint64_t)MBLS_SLOT_APK * 12 * ws.stride + pbase + p;
#pragma unroll 12
    for (int w = 0; w < 36; w++) dst[(uint64_t)w * ws.stride] = src[(uint64_t)w * ws.stride];
}
// One level of the per-message sums of the blinded keys (slot APK of the positions; wp = the workspace seen from the first position): the twin of k_g2_seg_tree_d
// on the generated G1 addition; lanes without a partner at this level return before the routine.
__global__ void MBLS_LB k_g1_seg_tree_d(mbls_ws wp, const uint32_t* map, const uint32_t* off, uint64_t n_msgs, uint64_t n, uint64_t half) {
#if MBLS_DEVICE_ASM
    const uint64_t p = gid();
    uint64_t lo, hi;
    if (!vms_owner_range(map, off, n_msgs, n, p, &lo, &hi)) return;
    if (!vmb_takes_partner(p, lo, hi, half)) return;
    g1_tree_d_call(wp, p, half, threadIdx.x);
#endif
}
// Miller item j < miller_items: H <- the table entry of message j (lane_h_gather; an empty list: the empty message's), APK <- the sum at the head of message
// j's range, infinity for a message no set names (its pair is skipped: it contributes 1). A listed message with a bad range rejects the check exactly when a
// set names it: its bit goes to the call's status word. Every slot the Miller loops read is written here.
__global__ void __launch_bounds__(MBLS_HB) k_vms_heads(mbls_ws ws, const uint32_t* tab, uint64_t tstride, const uint32_t* flags, const uint32_t* off, const uint32_t* cnt,
                                                       uint64_t n_msgs, uint64_t miller_items, uint64_t pbase, uint32_t* st_or) {
    const uint64_t j = (uint64_t)blockIdx.x * MBLS_HB + threadIdx.x; if (j >= miller_items) return;
    const uint32_t st = lane_h_gather(ws, j, tab, tstride, flags, (uint32_t)j, n_msgs);
    const bool some = j < n_msgs && cnt[j] != 0;
    const uint64_t it = pbase + (some ? (uint64_t)off[j] : 0);             // (the first position exists in every such workspace: a message without sets reads it and keeps nothing)
    g1j o; g1_set_inf(&o);
    g1j a; a.x = ws_ld(ws, MBLS_SLOT_APK, it); a.y = ws_ld(ws, MBLS_SLOT_APK + 1, it); a.z = ws_ld(ws, MBLS_SLOT_APK + 2, it);
    ws_st(ws, MBLS_SLOT_APK, j, fp_select(some, a.x, o.x)); ws_st(ws, MBLS_SLOT_APK + 1, j, fp_select(some, a.y, o.y)); ws_st(ws, MBLS_SLOT_APK + 2, j, fp_select(some, a.z, o.z));
    if (some && st) atomicOr(st_or, st);
}
// ---- verify_multiple over the RESIDENT message table (mbls_verify_multiple*_msgtable*): the grouping above runs with the table as the list (n_msgs = T, the
// table's size when the call is enqueued), and the table may hold far more entries than the call names -- so the Miller items are the entries that are NAMED,
// compacted on the device (mbls_vmt.h): flag[j] = cnt[j] != 0, roff = the exclusive scan of the flags (k_vms_scan over the flag words), named[roff[j]] = j.
// D = roff[T] stays on the device; the host sizes the Miller phase by a bound on it (vmt_bound).
__global__ void MBLS_LB k_vmt_flag(const uint32_t* cnt, uint64_t T, uint32_t* flag) {
    const uint64_t j = gid(); if (j >= T) return;
    flag[j] = vmt_flag(cnt[j]);
}
__global__ void MBLS_LB k_vmt_named(const uint32_t* flag, const uint32_t* roff, uint64_t T, uint32_t* named) {
    const uint64_t j = gid(); if (j >= T) return;
    uint32_t slot;
    if (vmt_named_slot(flag, roff, j, &slot) && (uint64_t)slot < T) named[slot] = (uint32_t)j;
}
// the twin of k_vms_heads. Miller item r < miller_items, D = *live: r < D -- H <- table entry named[r], APK <- the sum at the head of that entry's range (a
// flagged entry rejects the check: some set names it); otherwise the private entry and the point at infinity (the pair is skipped and contributes 1), and slot F
// <- 1, which is what a wave that returns early (k_coop_t's live count, k_vmt_miller) leaves for the product tree. Every slot the Miller loops read is written here.
__global__ void __launch_bounds__(MBLS_HB) k_vmt_heads(mbls_ws ws, const uint32_t* tab, uint64_t tstride, const uint32_t* flags, uint64_t T, const uint32_t* off,
                                                       const uint32_t* named, const uint32_t* live, uint64_t miller_items, uint64_t pbase, uint32_t* st_or) {
    const uint64_t r = (uint64_t)blockIdx.x * MBLS_HB + threadIdx.x; if (r >= miller_items) return;
    const uint64_t D = live[0];
    if (r == 0 && vmt_overflow(D, miller_items)) atomicOr(st_or, MBLS_ST_BAD_MSG_RANGE);      // fail closed (vmt_bound makes this unreachable)
    uint32_t idx; uint64_t pos;
    const bool some = vmt_head(named, off, D, r, &idx, &pos) && (uint64_t)idx < T;
    const uint32_t st = lane_h_gather(ws, r, tab, tstride, flags, some ? idx : MBLS_VMT_NO_ENTRY, T);
    const uint64_t it = pbase + (some ? pos : 0);
    g1j o; g1_set_inf(&o);
    g1j a; a.x = ws_ld(ws, MBLS_SLOT_APK, it); a.y = ws_ld(ws, MBLS_SLOT_APK + 1, it); a.z = ws_ld(ws, MBLS_SLOT_APK + 2, it);
    ws_st(ws, MBLS_SLOT_APK, r, fp_select(some, a.x, o.x)); ws_st(ws, MBLS_SLOT_APK + 1, r, fp_select(some, a.y, o.y)); ws_st(ws, MBLS_SLOT_APK + 2, r, fp_select(some, a.z, o.z));
    if (!some) {
        fp12 f; fp12_set_one(&f);
        const fp* one = &f.c0.c0.c0;
        for (int t = 0; t < 12; t++) ws_st(ws, MBLS_SLOT_F + t, r, one[t]);
    }
    if (some && st) atomicOr(st_or, st);
}
// the lane forms of the Miller loops over such Miller items (wv = the workspace seen from the launch's first item, which is Miller item `first`; cnt items):
// k_miller_single's and k_miller_single2's body for the items below the live count; a wave without one returns after one ballot, as the locate phase's waves
// without a candidate do -- it leaves its SIMD to the chains beside it, and whole idle rounds above a round of Miller items cost nothing (a call of one round
// is not shortened: its live waves still take the lane form's time)
template <int LPP> MBLS_FN void vmt_miller_body(const mbls_ws& wv, uint64_t cnt, uint64_t first, const uint32_t* live, uint32_t* spill) {
    const uint64_t t = LPP == 2 ? gid() >> 1 : gid();
    const bool on = t < cnt && !vmt_wave_idle(first + t, live[0]);
    if (!__ballot(on)) return;
    if (!on) return;
    miller_single_body<LPP>(wv, cnt, 0, 0, spill);
}
__global__ void MBLS_LB k_vmt_miller(mbls_ws wv, uint64_t cnt, uint64_t first, const uint32_t* live) {
    __shared__ uint32_t spill[154 * 64];
    vmt_miller_body<1>(wv, cnt, first, live, spill);
}
__global__ void MBLS_LB k_vmt_miller2(mbls_ws wv, uint64_t cnt, uint64_t first, const uint32_t* live) {
    __shared__ uint32_t spill[154 * 64];
    vmt_miller_body<2>(wv, cnt, first, live, spill);
}
// the tail: one final exponentiation per batch with verify_multiple's reject mask (lane_final<true>: the body of k_final / k_final2, the fold of final_fold_batch)
__global__ void MBLS_LB k_vmb_final(mbls_ws ws, uint32_t* status, uint8_t* results, uint64_t n) {
    __shared__ uint32_t accstore[154 * 64];
    uint64_t i = gid(); if (i >= n) return;
    uint32_t st = status[i]; uint8_t r; lane_final<true>(ws, i, &st, &r, (MBLS_LDS uint32_t*)accstore, threadIdx.x, true); status[i] = st; results[i] = r;
}
__global__ void MBLS_LB k_vmb_final2(mbls_ws ws, uint32_t* status, uint8_t* results, uint64_t n) {
    __shared__ uint32_t accstore[154 * 64];
    const uint64_t t = gid(); if (t >= 2 * n) return;
    const uint64_t i = t >> 1;
#if MBLS_DEVICE_ASM
    uint32_t st = status[i]; uint8_t r;
    lane_final2<true>(ws, i, &st, &r, (MBLS_LDS uint32_t*)accstore, threadIdx.x);
    if ((t & 1) == 0) { status[i] = st; results[i] = r; }
#endif
}
// ---- which sets of a rejected batch (mbls_verify_multiple_batches_locate*). The per-batch trees work in place and leave sums at range heads, so set i's blinded
// signature and Miller value are gone when its batch's verdict is known: a SHADOW item per set, workspace item sh + i behind everything phase one works on
// (mbls_vml.h vml_shadow_first), keeps them. Phase two then gives every set of a rejected batch the one-set batch's check, FE(f_i . ML(-G1, [r_i] sig_i)) = 1,
// on the lane bodies phase one runs. One wave per SIMD throughout: a wave without a candidate returns at once and costs nothing.
// before the signatures' trees: set i's [r_i] sig_i (slot S) -> the (sig, -G1) pair of its shadow item in the one-pair Miller kernels' operand layout
__global__ void MBLS_LB k_vml_keep_sig(mbls_ws ws, uint64_t n, uint64_t sh) {
    const uint64_t i = gid(); if (i >= n) return;
    ws_st2(ws, MBLS_SLOT_H, sh + i, ws_ld2(ws, MBLS_SLOT_S, i)); ws_st2(ws, MBLS_SLOT_H + 2, sh + i, ws_ld2(ws, MBLS_SLOT_S + 2, i));
    ws_st2(ws, MBLS_SLOT_H + 4, sh + i, ws_ld2(ws, MBLS_SLOT_S + 4, i));
    ws_st(ws, MBLS_SLOT_APK, sh + i, fp_load_const(MBLS_G1_X)); ws_st(ws, MBLS_SLOT_APK + 1, sh + i, fp_load_const(MBLS_G1_NEG_Y)); ws_st(ws, MBLS_SLOT_APK + 2, sh + i, fp_one());
}
// item `to` + i <- the Miller value of item `from` + i (12 Fp, word for word)
static __device__ __forceinline__ void vml_copy_f(const mbls_ws& ws, uint64_t from, uint64_t to) {
    const uint32_t* src = ws.w + (uint64_t)MBLS_SLOT_F * 12 * ws.stride + from;
    uint32_t* dst = ws.w + (uint64_t)MBLS_SLOT_F * 12 * ws.stride + to;
#pragma unroll 12
    for (int w = 0; w < 144; w++) dst[(uint64_t)w * ws.stride] = src[(uint64_t)w * ws.stride];
}
// before the products' trees: set i's Miller value f_i -> slot F of its shadow item
__global__ void MBLS_LB k_vml_keep_f(mbls_ws ws, uint64_t n, uint64_t sh) {
    const uint64_t i = gid(); if (i >= n) return;
    vml_copy_f(ws, i, sh + i);
}
// after the per-batch tail, one lane per set: the answer of every set that needs no pairing, and the candidate flags (the rule: mbls_vml.h vml_mark). A
// candidate's f_i moves back to slot F of the set's own item -- phase one is done with the items [0, n), and the shadow's slot F is where the Miller loop of
// its (sig, -G1) pair leaves g_i.
__global__ void MBLS_LB k_vml_mark(mbls_ws ws, const uint32_t* map, const uint32_t* off, uint32_t k, uint64_t B, uint64_t n, const uint32_t* st_set, const uint32_t* owned,
                                   const uint8_t* batch_results, uint32_t* cand, uint8_t* set_results, uint32_t* set_status, uint64_t sh) {
    const uint64_t i = gid(); if (i >= n) return;
    uint64_t lo = 0, hi = 0, b = 0;
    bool own = vmb_owner_range(map, off, k, B, n, i, &lo, &hi);
    if (own) { b = off ? map[i] : i / k; own = vmb_owns_all(off ? owned : nullptr, b, lo, hi); }
    uint32_t st;
    const uint32_t v = vml_mark(own, own && batch_results[b] != 0, st_set[i], &st);
    cand[i] = v == MBLS_VML_CANDIDATE ? 1u : 0u;
    set_results[i] = v == MBLS_VML_TRUE ? 1 : 0;                  // (a candidate stays 0 until its own check has spoken: fail closed)
    if (set_status) set_status[i] = st;
    if (v == MBLS_VML_CANDIDATE) vml_copy_f(ws, sh + i, i);
}
// g_i = Miller([r_i] sig_i, -G1) over the shadow items (wsh = the workspace seen from the first shadow item of the launch), candidates only: k_miller_single's
// and k_miller_single2's body
template <int LPP> MBLS_FN void vml_miller_body(const mbls_ws& wsh, uint64_t n, const uint32_t* cand, uint32_t* spill) {
    const uint64_t i = LPP == 2 ? gid() >> 1 : gid();
    const bool on = i < n && cand[i] != 0;
    if (!__ballot(on)) return;
    if (!on) return;
    miller_single_body<LPP>(wsh, n, 0, 0, spill);
}
__global__ void MBLS_LB k_vml_miller(mbls_ws wsh, uint64_t n, const uint32_t* cand) {
    __shared__ uint32_t spill[154 * 64];
    vml_miller_body<1>(wsh, n, cand, spill);
}
__global__ void MBLS_LB k_vml_miller2(mbls_ws wsh, uint64_t n, const uint32_t* cand) {
    __shared__ uint32_t spill[154 * 64];
    vml_miller_body<2>(wsh, n, cand, spill);
}
// item i <- f_i . g_i (slot F of item i times slot F of its shadow item sh + i: the generated tree routine with the shadow as the partner), candidates only
__global__ void MBLS_LB k_vml_product(mbls_ws ws, uint64_t n, uint64_t sh, const uint32_t* cand) {
#if MBLS_DEVICE_ASM
    __shared__ uint32_t spill[154 * 64];
    const uint64_t i = gid();
    const bool on = i < n && cand[i] != 0;
    if (!__ballot(on)) return;
    if (!on) return;
    tree_level_d_call<false>(ws, i, sh, (MBLS_LDS uint32_t*)spill, threadIdx.x);
#endif
}
// the candidates' verdicts: one final exponentiation per candidate with verify_multiple's reject mask on the set's OWN word (k_vmb_final's body; the word
// carries no rejecting bit, or the set would be no candidate, so MBLS_ST_PAIRING_FAILED is added exactly where the check fails)
__global__ void MBLS_LB k_vml_final(mbls_ws ws, const uint32_t* st_set, const uint32_t* cand, uint8_t* set_results, uint32_t* set_status, uint64_t n) {
    __shared__ uint32_t accstore[154 * 64];
    const uint64_t i = gid();
    const bool on = i < n && cand[i] != 0;
    if (!__ballot(on)) return;
    if (!on) return;
    uint32_t st = st_set[i]; uint8_t r; lane_final<true>(ws, i, &st, &r, (MBLS_LDS uint32_t*)accstore, threadIdx.x, true);
    set_results[i] = r; if (set_status) set_status[i] = st;
}
__global__ void MBLS_LB k_vml_final2(mbls_ws ws, const uint32_t* st_set, const uint32_t* cand, uint8_t* set_results, uint32_t* set_status, uint64_t n) {
    __shared__ uint32_t accstore[154 * 64];
    const uint64_t t = gid();
    const uint64_t i = t >> 1;
    const bool on = i < n && cand[i] != 0;
    if (!__ballot(on)) return;
    if (!on) return;
#if MBLS_DEVICE_ASM
    uint32_t st = st_set[i]; uint8_t r;
    lane_final2<true>(ws, i, &st, &r, (MBLS_LDS uint32_t*)accstore, threadIdx.x);
    if ((t & 1) == 0) { set_results[i] = r; if (set_status) set_status[i] = st; }
#endif
}
// ---- which sets of a rejected call over a shared message list (mbls_verify_multiple*_shared_msgs_locate*). The per-set route has a Miller value per set and is
// the scheme above with the call as the one batch. The GROUPED route never computes f_i = ML([r_i] apk_i, H(m_i)) -- one value per message exists --, its heads
// and trees overwrite the sets' blinded keys and the signatures' tree their slot S: each set gets TWO shadow items behind everything phase one uses (mbls_vsl.h),
// A(i) = sh + i for the pair (H(m_i), [r_i] apk_i) and B(i) = sh + n + i for ([r_i] sig_i, -G1; k_vml_keep_sig), and phase two walks both pairs' Miller loops.
// behind k_blind_g1_d, before the scatter's positions are summed and the heads written: set i's [r_i] apk_i (slot APK, Jacobian) -> slot APK of A(i)
__global__ void MBLS_LB k_vsl_keep_key(mbls_ws ws, uint64_t n, uint64_t sh) {
    const uint64_t i = gid(); if (i >= n) return;
    const uint32_t* src = ws.w + (uint64_t)MBLS_SLOT_APK * 12 * ws.stride + i;
    uint32_t* dst = ws.w + (uint64_t)MBLS_SLOT_APK * 12 * ws.stride + sh + i;
#pragma unroll 12
    for (int w = 0; w < 36; w++) dst[(uint64_t)w * ws.stride] = src[(uint64_t)w * ws.stride];
}
// after the call's tail, one lane per set (wsa = the workspace seen from A(0)): the answer of every set that needs no pairing and the candidate flags (the
// rule: mbls_vsl.h vsl_mark -- the call's verdict, the set's own word, the bad-range flag of the message the set names, looked up through msg_idx[i]). A
// candidate names a sound message of the list: its point goes from the table to slot H of A(i) (lane_h_gather), which completes the pair.
__global__ void MBLS_LB k_vsl_mark(mbls_ws wsa, const uint32_t* tab, uint64_t tstride, const uint32_t* flags, const uint32_t* msg_idx, uint64_t n_msgs, uint64_t n,
                                   const uint32_t* st_set, const uint8_t* call_result, uint32_t* cand, uint8_t* set_results, uint32_t* set_status) {
    const uint64_t i = gid(); if (i >= n) return;
    const uint32_t j = msg_idx[i];
    uint32_t st;
    const uint32_t v = vsl_mark(call_result[0] != 0, st_set[i], j, n_msgs, flags, &st);
    cand[i] = v == MBLS_VML_CANDIDATE ? 1u : 0u;
    set_results[i] = v == MBLS_VML_TRUE ? 1 : 0;                  // (a candidate stays 0 until its own check has spoken: fail closed)
    if (set_status) set_status[i] = st;
    if (v == MBLS_VML_CANDIDATE) (void)lane_h_gather(wsa, i, tab, tstride, flags, j, n_msgs);
}
// the Miller loops of the candidates' shadow pairs, ONE launch over the shadow items -- 2 n on the grouped route, both pairs of every set; n on the per-set
// route -- (wv = the workspace seen from the launch's first item, which is item `first` of the shadows; cnt items): k_miller_single's and k_miller_single2's
// body, the flag read at the item's set (vsl_shadow_set)
template <int LPP> MBLS_FN void vsl_miller_body(const mbls_ws& wv, uint64_t cnt, uint64_t first, uint64_t n, const uint32_t* cand, uint32_t* spill) {
    const uint64_t t = LPP == 2 ? gid() >> 1 : gid();
    const bool on = t < cnt && cand[vsl_shadow_set(first + t, n)] != 0;
    if (!__ballot(on)) return;
    if (!on) return;
    miller_single_body<LPP>(wv, cnt, 0, 0, spill);
}
__global__ void MBLS_LB k_vsl_miller(mbls_ws wv, uint64_t cnt, uint64_t first, uint64_t n, const uint32_t* cand) {
    __shared__ uint32_t spill[154 * 64];
    vsl_miller_body<1>(wv, cnt, first, n, cand, spill);
}
__global__ void MBLS_LB k_vsl_miller2(mbls_ws wv, uint64_t cnt, uint64_t first, uint64_t n, const uint32_t* cand) {
    __shared__ uint32_t spill[154 * 64];
    vsl_miller_body<2>(wv, cnt, first, n, cand, spill);
}
// verify_multiple over several devices ("one exchange step"): what one shard contributes is the product of its
// sets' Miller values (slot F of item 0), its sum of blinded signatures (slot S of item 0) and the OR of its status words -- a
// MBLS_VM_PARTIAL_BYTES record in the workspace's own number format (opaque: only mbls_verify_multiple_finish_device of the same build reads
// it). An empty shard contributes (1, infinity, 0).
#define MBLS_VM_PARTIAL_WORDS (MBLS_VM_PARTIAL_BYTES / 4)
#define MBLS_VM_MAGIC 0x4d564d31u
static_assert(MBLS_VM_PARTIAL_WORDS >= 18 * 12 + 2, "partial record too small");
__global__ void MBLS_LB k_vm_export(mbls_ws ws, const uint32_t* st_or, int empty, uint32_t* out) {
    const uint32_t t = threadIdx.x;
    if (blockIdx.x) return;
    if (empty) {
        if (t == 0) {
            fp12 f; fp12_set_one(&f); const fp* one = &f.c0.c0.c0;
            for (int a = 0; a < 12; a++) for (int j = 0; j < 12; j++) out[12 * a + j] = one[a][j];
            for (int j = 144; j < 216; j++) out[j] = 0;                   // Z = 0: infinity
            out[216] = 0; out[217] = MBLS_VM_MAGIC;
            for (int j = 218; j < (int)MBLS_VM_PARTIAL_WORDS; j++) out[j] = 0;
        }
        return;
    }
    for (uint32_t j = t; j < 216; j += WG) {                             // word j of the record = limb j % 12 of slot F + j / 12 (F and S are adjacent)
        const uint32_t slot = MBLS_SLOT_F + j / 12, limb = j % 12;
        out[j] = ws.w[((uint64_t)slot * 12 + limb) * ws.stride];
    }
    if (t == 0) { out[216] = st_or[0]; out[217] = MBLS_VM_MAGIC; }
    for (uint32_t j = 218 + t; j < MBLS_VM_PARTIAL_WORDS; j += WG) out[j] = 0;
}
static_assert(MBLS_SLOT_S == MBLS_SLOT_F + 12, "k_vm_export / k_vm_import copy slots F and S as one range");
// record g -> slots F, S of item g; the status words ORed into st_or[0]; a record that is not one (wrong magic, or a coefficient of the Miller value that is
// not below p) makes the check fail. The range check is what lets the product tree's routine be generated for canonical words (tools/gen_tower_d.py G_CANON_IN):
// k_vm_export only ever writes such values, so a record that fails it was not made by this library; its Miller value is replaced by zeros, which are in range.
__global__ void MBLS_LB k_vm_import(mbls_ws ws, const uint32_t* in, uint64_t G, uint32_t* st_or) {
    const uint64_t g = gid(); if (g >= G) return;
    const uint32_t* r = in + g * MBLS_VM_PARTIAL_WORDS;
    bool wide = false;
    for (uint32_t a = 0; a < 12; a++) {
        int cmp = 0;                                                     // the sign of value - p, decided at the highest limb that differs
        for (int j = 11; j >= 0 && cmp == 0; j--) { const uint32_t w = r[12 * a + j], pl = fp_plimb(j); cmp = w > pl ? 1 : (w < pl ? -1 : 0); }
        wide |= cmp >= 0;
    }
    for (uint32_t j = 0; j < 216; j++) ws.w[((uint64_t)(MBLS_SLOT_F + j / 12) * 12 + j % 12) * ws.stride + g] = (wide && j < 144) ? 0u : r[j];
    uint32_t st = r[216];
    if (r[217] != MBLS_VM_MAGIC || wide) st |= MBLS_ST_PAIRING_FAILED | MBLS_ST_BAD_SIG_ENCODING;
    if (st) atomicOr(st_or, st);
}
// the signature k_sig decoded into slots 3..6 of item `item` (affine; y = 0: infinity) -> slot S of the same item in Jacobian form: the
// (sig, -G1) pair of aggregate_verify (reference src/aggregates.rs:158-164)
__global__ void MBLS_LB k_sigslot_to_s(mbls_ws ws, uint64_t item) {
    if (gid() != 0) return;
    g2j s; s.x = ws_ld2(ws, MBLS_SLOT_SIG, item); s.y = ws_ld2(ws, MBLS_SLOT_SIG + 2, item); s.z = fp2_one();
    if (fp2_is_zero(s.y)) g2_set_inf(&s);
    ws_st2(ws, MBLS_SLOT_S, item, s.x); ws_st2(ws, MBLS_SLOT_S + 2, item, s.y); ws_st2(ws, MBLS_SLOT_S + 4, item, s.z);
}

// ------------------------------------------------------------------------------------------------ auxiliary kernels
__global__ void MBLS_LB k_g1_decode(const uint8_t* in, int fmt, int validate, uint64_t n, uint8_t* out96, uint8_t* err) { uint64_t i = gid(); if (i < n) op_g1_decode(i, in, fmt, validate, out96, err); }
__global__ void MBLS_LB k_g1_key_validate(const uint8_t* in96, uint64_t n, uint8_t* ok) { uint64_t i = gid(); if (i < n) op_g1_key_validate(i, in96, ok); }
__global__ void MBLS_LB k_g1_compress(const uint8_t* in96, uint64_t n, uint8_t* out48, uint8_t* err) { uint64_t i = gid(); if (i < n) op_g1_compress(i, in96, out48, err); }
// n x Signature::from_bytes (reference src/signature.rs:43-46) + the subgroup test verify performs (:29): the decoder inlined as in k_sig and the GENERATED subgroup
// routine on the item's workspace slots (psi(P) = [x] P; no lane-private memory). err[i] = the decoder's code; in_g2 (optional): 1 for points of G2 and for infinity.
__global__ void MBLS_LB k_g2_check(mbls_ws ws, const uint8_t* in96, uint64_t n, uint8_t* err, uint8_t* in_g2) {
#if MBLS_DEVICE_ASM
    __shared__ uint32_t spill[154 * 64];
    uint64_t i = gid(); if (i >= n) return;
    fp2 x, y; bool inf;
    const int e = g2_decode_compressed_t<true>(&x, &y, &inf, in96 + 96 * i);
    err[i] = (uint8_t)e;
    if (!in_g2) return;                               // (uniform: a kernel argument)
    if (e) inf = true;
    if (inf) { x = fp2_zero(); y = fp2_zero(); }
    ws_st2(ws, MBLS_SLOT_SIG, i, x); ws_st2(ws, MBLS_SLOT_SIG + 2, i, y);
    const uint32_t fl = g2_group_d_call<false>(ws, i, (MBLS_LDS uint32_t*)spill, threadIdx.x);
    in_g2[i] = (!e && ((fl & 1u) | (inf ? 1u : 0u))) ? 1 : 0;
#endif
}
__global__ void MBLS_LB k_g2_add(const uint8_t* a, const uint8_t* b, uint64_t n, uint8_t* out, uint8_t* err) { uint64_t i = gid(); if (i < n) op_g2_add(i, a, b, out, err); }
__global__ void MBLS_LB k_g1_add(const uint8_t* a, const uint8_t* b, uint64_t n, uint8_t* out, uint8_t* err) { uint64_t i = gid(); if (i < n) op_g1_add(i, a, b, out, err); }
__global__ void MBLS_LB k_sk_to_pk(const uint8_t* sks, int fmt, uint64_t n, uint8_t* out) { uint64_t i = gid(); if (i < n) op_sk_to_pk(i, sks, fmt, out); }
__global__ void MBLS_LB k_fp_mul(const uint8_t* a, const uint8_t* b, uint64_t n, uint8_t* out, int op) { uint64_t i = gid(); if (i < n) op_fp_mul(i, n, a, b, out, op); }
// Raw-register probe of the digit-form leaves and passes (tools/gen_tower_d.py probe_ops): lane i runs ONE generated body on the register contents in[w n + i] and
// stores the registers the probe lists to out[w n + i]; tests/test_gpu_dform.py compares them with the CPU interpreter of the same instructions. The generated text
// loads and stores its own registers (SADDR form, like the routines' workspace traffic): nothing here sits between the test's integers and the body.
#if MBLS_DEVICE_ASM
#define MBLS_DFORM_PROBE_CASE(k, body) case k: asm volatile(body : "+{s66}"(ilo), "+{s67}"(ihi), "+{s68}"(olo), "+{s69}"(ohi) : "{v252}"(off), "{s70}"(st4) : MBLS_DFORM_PROBE_CLOBBERS); break;
#endif
__global__ void MBLS_LB k_dform_probe(const int32_t* in, int32_t* out, uint64_t n, int op, uint32_t* ran) {
    const uint64_t i = gid(); if (i >= n) return;
#if MBLS_DEVICE_ASM
    if (i == 0) *ran = 1u;                                                               // a build without the generated routines leaves it 0: the host reports that
    const uint32_t off = (uint32_t)(4 * i);                                              // n <= 2^24: every byte offset fits 32 bits
    uint32_t ilo = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)in), ihi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)(uintptr_t)in >> 32));
    uint32_t olo = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)out), ohi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)(uintptr_t)out >> 32));
    const uint32_t st4 = __builtin_amdgcn_readfirstlane((uint32_t)(4 * n));
    switch (op) {
        MBLS_DFORM_PROBE_EACH(MBLS_DFORM_PROBE_CASE)
        default: break;
    }
#endif
}
// PublicKey::from_secret_key as a key sum: [sk] G1 = sum_j [d_j 16^j] G1 over the 64 hexadecimal digits of sk, every term a record of a
// fixed 64 x 16 table (record 16 j + d; d = 0 is the point at infinity) -- the indexed key-sum routine does the rest, no doubling at all
__global__ void MBLS_LB k_sk_digits(const uint8_t* sks32, uint64_t n, uint32_t* idx) {
    uint64_t i = gid(); if (i >= n) return;
    const uint8_t* b = sks32 + 32 * i;
    for (uint32_t j = 0; j < 64; j++) {
        const uint32_t d = (b[31 - (j >> 1)] >> (4 * (j & 1))) & 15u;
        idx[64 * i + j] = 16 * j + d;
    }
}
// CONSTANT-TIME sk -> pk (the default; reference src/keys.rs:124-137 -- amcl's g1mul selects in constant time): lane (key i, window j) reads ALL 16 records
// [d 16^j] G1 of its window and keeps record d_j by selection, so neither an address nor the instruction stream depends on the key; the selected records form a
// per-batch table sel[64 i + j] that the key-sum routine then walks with the public indices 64 i + j (idx).
__global__ void __launch_bounds__(WG) k_sk_select(const uint8_t* sks32, uint64_t n, const uint32_t* gtab, uint32_t* sel, uint32_t* idx) {
    const uint64_t t = gid(); if (t >= 64 * n) return;
    const uint64_t i = t >> 6; const uint32_t j = (uint32_t)(t & 63);
    const uint32_t d = (sks32[32 * i + 31 - (j >> 1)] >> (4 * (j & 1))) & 15u;
    const uint4* rec = (const uint4*)(gtab + (size_t)16 * j * MBLS_KEYREC_DWORDS);
    uint4 acc[MBLS_KEYREC_DWORDS / 4];
#pragma unroll
    for (int q = 0; q < MBLS_KEYREC_DWORDS / 4; q++) acc[q] = rec[q];
    for (uint32_t e = 1; e < 16; e++) {
        // the selection as mask arithmetic on an OPAQUE mask: with a plain `take ? v : acc` the compiler guards the loads with the condition (s_and_saveexec +
        // s_cbranch_execz around global_load: only the lanes whose digit is e would touch record e -- exactly the access pattern this kernel exists to avoid).
        // tests/test_build_cpu.py checks the ISA: 16 x 8 unconditional 16-byte loads, no branch between the first load and the store.
        uint32_t m = 0u - (uint32_t)(e == d);
        asm volatile("" : "+v"(m));
#pragma unroll
        for (int q = 0; q < MBLS_KEYREC_DWORDS / 4; q++) {
            const uint4 v = rec[(size_t)e * (MBLS_KEYREC_DWORDS / 4) + q];
            acc[q].x = (v.x & m) | (acc[q].x & ~m); acc[q].y = (v.y & m) | (acc[q].y & ~m);
            acc[q].z = (v.z & m) | (acc[q].z & ~m); acc[q].w = (v.w & m) | (acc[q].w & ~m);
        }
    }
    uint4* out = (uint4*)(sel + t * MBLS_KEYREC_DWORDS);
#pragma unroll
    for (int q = 0; q < MBLS_KEYREC_DWORDS / 4; q++) out[q] = acc[q];
    idx[t] = (uint32_t)t;
}
__global__ void MBLS_LB k_apk_export_fmt(mbls_ws ws, uint64_t n, int fmt, uint8_t* out) {
    uint64_t i = gid(); if (i >= n) return;
    g1j a; a.x = ws_ld(ws, MBLS_SLOT_APK, i); a.y = ws_ld(ws, MBLS_SLOT_APK + 1, i); a.z = ws_ld(ws, MBLS_SLOT_APK + 2, i);
    fp x, y; bool inf; g1_to_affine(&x, &y, &inf, &a);
    if (fmt == MBLS_PK_COMPRESSED) g1_encode_compressed(out + 48 * i, x, y, inf); else g1_encode_uncompressed(out + 96 * i, x, y, inf);
}
__global__ void MBLS_LB k_apk_export(mbls_ws ws, uint64_t n, uint8_t* out96) { uint64_t i = gid(); if (i < n) op_apk_export(ws, i, out96); }
// H(m) as the message phase of the pipeline left it in workspace slots 7..12 (Jacobian) -> 96 compressed bytes (the probe mbls_hash_to_g2_batch)
// Signature::new (reference src/signature.rs:17-21) on the generated routines. psi acts on G2 as multiplication by the curve parameter
// x = -y, y = 0xd201000000010000, and r = y^4 - y^2 + 1 < y^4: with sk mod r = a0 + a1 y + a2 y^2 + a3 y^3 (0 <= a_j < y < 2^64),
// [sk] H = sum_j [a_j] (-1)^j psi^j(H) -- four 64-bit multiplications that run side by side on four lanes (items i, n + i, 2n + i, 3n + i)
// with verify_multiple's windowed routine (g2_blind_routine without its subgroup test), then two levels of the G2 sum tree.
// (64-bit limbs in named variables, every limb loop unrolled: nothing here is indexed at run time, so nothing lives in lane-private memory)
MBLS_FN uint64_t div_step_y(uint64_t* rem, uint64_t limb) {       // (rem : limb) / y with rem < y: the quotient limb, the remainder left in *rem (restoring, one bit a step)
    const uint64_t y = MBLS_X_ABS;
    uint64_t r = *rem, q = 0;
    for (int b = 63; b >= 0; b--) {
        const uint64_t top = r >> 63;
        r = (r << 1) | ((limb >> b) & 1u);
        const bool ge = top | (r >= y);
        r = ge ? r - y : r; q = (q << 1) | (ge ? 1u : 0u);
    }
    *rem = r; return q;
}
MBLS_FN void scalar_base_y_digits(uint64_t a[4], const uint8_t* sk32) {
    uint64_t k3 = 0, k2 = 0, k1 = 0, k0 = 0;                        // big-endian bytes -> limbs, k0 the least significant
#pragma unroll
    for (int j = 0; j < 8; j++) { k3 = (k3 << 8) | sk32[j]; k2 = (k2 << 8) | sk32[8 + j]; k1 = (k1 << 8) | sk32[16 + j]; k0 = (k0 << 8) | sk32[24 + j]; }
    const uint64_t r0 = 0xffffffff00000001ull, r1 = 0x53bda402fffe5bfeull, r2 = 0x3339d80809a1d805ull, r3 = 0x73eda753299d7d48ull;      // the group order
#pragma unroll
    for (int rep = 0; rep < 4; rep++) {                            // any 32-byte value: 2^256 < 5 r, at most four subtractions
        const uint64_t d0 = k0 - r0; const uint64_t b0 = k0 < r0;
        const uint64_t t1 = k1 - r1; const uint64_t d1 = t1 - b0; const uint64_t b1 = (k1 < r1) | (t1 < b0);
        const uint64_t t2 = k2 - r2; const uint64_t d2 = t2 - b1; const uint64_t b2 = (k2 < r2) | (t2 < b1);
        const uint64_t t3 = k3 - r3; const uint64_t d3 = t3 - b2; const uint64_t b3 = (k3 < r3) | (t3 < b2);
        k0 = b3 ? k0 : d0; k1 = b3 ? k1 : d1; k2 = b3 ? k2 : d2; k3 = b3 ? k3 : d3;
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {                                  // k <- k / y, a[t] = k mod y
        uint64_t rem = 0;
        k3 = div_step_y(&rem, k3); k2 = div_step_y(&rem, k2); k1 = div_step_y(&rem, k1); k0 = div_step_y(&rem, k0);
        a[t] = rem;
    }
}
__global__ void MBLS_LB k_sign_blind(mbls_ws ws, const uint8_t* sks32, uint64_t n, int ct) {
#if MBLS_DEVICE_ASM
    __shared__ uint32_t spill[154 * 64];
    uint64_t t = gid(); if (t >= 4 * n) return;
    const uint64_t i = t % n; const uint32_t j = (uint32_t)(t / n);
    g2j h; h.x = ws_ld2(ws, MBLS_SLOT_H, i); h.y = ws_ld2(ws, MBLS_SLOT_H + 2, i); h.z = ws_ld2(ws, MBLS_SLOT_H + 4, i);
    fp2 x, y; bool inf; g2_to_affine(&x, &y, &inf, &h);           // H(m) is never infinity in practice; (0, 0) with the scalar 0 if it is
    g2j q; q.x = x; q.y = y; q.z = fp2_one();
    for (uint32_t e = 0; e < 3; e++) { g2j u; g2_psi(&u, &q); const bool on = e < j; q.x = fp2_select(on, u.x, q.x); q.y = fp2_select(on, u.y, q.y); }
    q.y = fp2_select((j & 1u) != 0, fp2_neg(q.y), q.y);
    if (inf) { q.x = fp2_zero(); q.y = fp2_zero(); }
    ws_st2(ws, MBLS_SLOT_SIG, t, q.x); ws_st2(ws, MBLS_SLOT_SIG + 2, t, q.y);
    uint64_t a[4]; scalar_base_y_digits(a, sks32 + 32 * i);
    const uint64_t r = j == 0 ? a[0] : j == 1 ? a[1] : j == 2 ? a[2] : a[3];
    // ct (the default): the window tables are read by scan + selection, never at an address that depends on the key (mbls_ctx_set_secret_ops)
    if (ct) (void)g2_blind_ct_d_call(ws, t, (MBLS_LDS uint32_t*)spill, threadIdx.x, inf ? 0 : r, 1u);
    else (void)g2_blind_d_call(ws, t, (MBLS_LDS uint32_t*)spill, threadIdx.x, inf ? 0 : r, 1u);
#endif
}
__global__ void MBLS_LB k_s_export(mbls_ws ws, uint64_t n, uint8_t* out96) {
    uint64_t i = gid(); if (i >= n) return;
    g2j h; h.x = ws_ld2(ws, MBLS_SLOT_S, i); h.y = ws_ld2(ws, MBLS_SLOT_S + 2, i); h.z = ws_ld2(ws, MBLS_SLOT_S + 4, i);
    g2_encode_jacobian(out96 + 96 * i, &h);
}
__global__ void MBLS_LB k_h_export(mbls_ws ws, uint64_t n, uint8_t* out96) {
    uint64_t i = gid(); if (i >= n) return;
    g2j h; h.x = ws_ld2(ws, MBLS_SLOT_H, i); h.y = ws_ld2(ws, MBLS_SLOT_H + 2, i); h.z = ws_ld2(ws, MBLS_SLOT_H + 4, i);
    g2_encode_jacobian(out96 + 96 * i, &h);
}
__global__ void MBLS_LB k_fp_mul_bench(uint32_t* sink, uint32_t iters, uint64_t n) {
    uint64_t i = gid(); if (i >= n) return;
    fp a = fp_load_const(MBLS_G1_X), b = fp_load_const(MBLS_G1_Y);
    a[0] ^= (uint32_t)i;
    for (uint32_t it = 0; it < iters; it++) a = fp_mul(a, b);
    uint32_t acc = 0;
    for (int j = 0; j < 12; j++) acc ^= a[j];
    sink[i] = acc;
}

// VALU issue-rate calibration (bench.py, valu_issue): 128 instructions per iteration, 8 independent chains per lane.
// mode 0: v_mad_u64_u32 with the carry-out alternating between VCC and SGPR pairs (what the multiplication routines issue);
// mode 1: v_add_co / v_addc chains (the class every other integer instruction of the routines issues at).
#define MBLS_REP4(x) x x x x
#define MBLS_VB_V8(a) "v" #a "0", "v" #a "1", "v" #a "2", "v" #a "3", "v" #a "4", "v" #a "5", "v" #a "6", "v" #a "7", "v" #a "8", "v" #a "9"
#define MBLS_VALU_BENCH_CLOBBERS "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", MBLS_VB_V8(1), MBLS_VB_V8(2), MBLS_VB_V8(3), MBLS_VB_V8(4), MBLS_VB_V8(5), \
    MBLS_VB_V8(6), MBLS_VB_V8(7), MBLS_VB_V8(8), MBLS_VB_V8(9), MBLS_VB_V8(10), MBLS_VB_V8(11), "v120", "v121", "v122", "v123", "v124", "v125", \
    "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65", "vcc", "scc"
#define MBLS_REP16(x) MBLS_REP4(MBLS_REP4(x))
__global__ void __launch_bounds__(WG) k_valu_bench(uint32_t* sink, uint32_t iters, int mode) {
    uint32_t a = (threadIdx.x * 2654435761u + blockIdx.x) | 1u, b = a ^ 0x9e3779b9u;
    uint64_t c0 = a, c1 = b, c2 = a + 1, c3 = b + 1, c4 = a + 2, c5 = b + 2, c6 = a + 3, c7 = b + 3;
    uint32_t h0 = a, h1 = b, h2 = a + 5, h3 = b + 7;
    for (uint32_t i = 0; i < iters; i++) {
        if (mode == 0) {
            MBLS_REP16(asm volatile("v_mad_u64_u32 %0, vcc, %8, %9, %0\n v_mad_u64_u32 %1, s[20:21], %8, %9, %1\n v_mad_u64_u32 %2, vcc, %8, %9, %2\n v_mad_u64_u32 %3, s[22:23], %8, %9, %3\n"
                                    "v_mad_u64_u32 %4, vcc, %8, %9, %4\n v_mad_u64_u32 %5, s[20:21], %8, %9, %5\n v_mad_u64_u32 %6, vcc, %8, %9, %6\n v_mad_u64_u32 %7, s[22:23], %8, %9, %7\n"
                                    : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b) : "vcc", "s20", "s21", "s22", "s23");)
        } else if (mode == 2) {
#if MBLS_DEVICE_ASM
            // the Fp2 product routine itself, eight times back to back (8 x 1 281 instructions, 980 of them multiply-accumulates): what a kernel
            // made of nothing but products would issue at -- the reference the generated kernels' rates are quoted against
            MBLS_REP4(asm volatile(MBLS_FP2_MUL_D_ASM MBLS_FP2_MUL_D_ASM ::: MBLS_VALU_BENCH_CLOBBERS);)
#endif
        } else if (mode == 3) {
#if MBLS_DEVICE_ASM
            // the same with the paired Fp product of the key-sum routines (8 x 923 instructions, 784 multiply-accumulates each)
            MBLS_REP4(asm volatile(MBLS_FP_MULPAIR_D_ASM MBLS_FP_MULPAIR_D_ASM ::: MBLS_VALU_BENCH_CLOBBERS);)
#endif
        } else if (mode == 4) {
            // class model against mix, the experiment: 8 multiply-accumulates and 4 plain two-operand operations INTERLEAVED 2 : 1 (the kernels'
            // proportion) ...
            MBLS_REP16(asm volatile("v_mad_u64_u32 %0, vcc, %12, %13, %0\n v_mad_u64_u32 %1, s[20:21], %12, %13, %1\n v_add_u32_e32 %8, %12, %8\n"
                                    "v_mad_u64_u32 %2, vcc, %12, %13, %2\n v_mad_u64_u32 %3, s[22:23], %12, %13, %3\n v_and_b32_e32 %9, %13, %9\n"
                                    "v_mad_u64_u32 %4, vcc, %12, %13, %4\n v_mad_u64_u32 %5, s[20:21], %12, %13, %5\n v_add_u32_e32 %10, %13, %10\n"
                                    "v_mad_u64_u32 %6, vcc, %12, %13, %6\n v_mad_u64_u32 %7, s[22:23], %12, %13, %7\n v_xor_b32_e32 %11, %12, %11\n"
                                    : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7), "+v"(h0), "+v"(h1), "+v"(h2), "+v"(h3)
                                    : "v"(a), "v"(b) : "vcc", "s20", "s21", "s22", "s23");)
        } else if (mode == 5) {
            // ... and the SAME twelve instructions in two homogeneous blocks (what a per-class model of the stream assumes)
            MBLS_REP16(asm volatile("v_mad_u64_u32 %0, vcc, %12, %13, %0\n v_mad_u64_u32 %1, s[20:21], %12, %13, %1\n"
                                    "v_mad_u64_u32 %2, vcc, %12, %13, %2\n v_mad_u64_u32 %3, s[22:23], %12, %13, %3\n"
                                    "v_mad_u64_u32 %4, vcc, %12, %13, %4\n v_mad_u64_u32 %5, s[20:21], %12, %13, %5\n"
                                    "v_mad_u64_u32 %6, vcc, %12, %13, %6\n v_mad_u64_u32 %7, s[22:23], %12, %13, %7\n"
                                    "v_add_u32_e32 %8, %12, %8\n v_and_b32_e32 %9, %13, %9\n v_add_u32_e32 %10, %13, %10\n v_xor_b32_e32 %11, %12, %11\n"
                                    : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7), "+v"(h0), "+v"(h1), "+v"(h2), "+v"(h3)
                                    : "v"(a), "v"(b) : "vcc", "s20", "s21", "s22", "s23");)
        } else if (mode == 7) {
            // the scans' own instruction: v_mad_i64_i32 on eight accumulators (the peak of bench.py's mac_frac: whichever of mode 0 and this one issues faster)
            MBLS_REP16(asm volatile("v_mad_i64_i32 %0, vcc, %8, %9, %0\n v_mad_i64_i32 %1, s[20:21], %8, %9, %1\n v_mad_i64_i32 %2, vcc, %8, %9, %2\n v_mad_i64_i32 %3, s[22:23], %8, %9, %3\n"
                                    "v_mad_i64_i32 %4, vcc, %8, %9, %4\n v_mad_i64_i32 %5, s[20:21], %8, %9, %5\n v_mad_i64_i32 %6, vcc, %8, %9, %6\n v_mad_i64_i32 %7, s[22:23], %8, %9, %7\n"
                                    : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b) : "vcc", "s20", "s21", "s22", "s23");)
        } else if (mode == 6) {
            // ... and the four plain operations alone
            MBLS_REP16(asm volatile("v_add_u32_e32 %0, %4, %0\n v_and_b32_e32 %1, %5, %1\n v_add_u32_e32 %2, %5, %2\n v_xor_b32_e32 %3, %4, %3\n"
                                    "v_add_u32_e32 %0, %5, %0\n v_and_b32_e32 %1, %4, %1\n v_add_u32_e32 %2, %4, %2\n v_xor_b32_e32 %3, %5, %3\n"
                                    : "+v"(h0), "+v"(h1), "+v"(h2), "+v"(h3) : "v"(a), "v"(b));)
        } else {
            MBLS_REP16(asm volatile("v_add_co_u32_e64 %0, vcc, %4, %0\n v_add_co_u32_e64 %2, s[20:21], %5, %2\n v_addc_co_u32_e64 %1, vcc, %5, %1, vcc\n v_addc_co_u32_e64 %3, s[20:21], %4, %3, s[20:21]\n"
                                    "v_add_co_u32_e64 %0, vcc, %5, %0\n v_add_co_u32_e64 %2, s[20:21], %4, %2\n v_addc_co_u32_e64 %1, vcc, %4, %1, vcc\n v_addc_co_u32_e64 %3, s[20:21], %5, %3, s[20:21]\n"
                                    : "+v"(h0), "+v"(h1), "+v"(h2), "+v"(h3) : "v"(a), "v"(b) : "vcc", "s20", "s21");)
        }
    }
    sink[(uint64_t)blockIdx.x * WG + threadIdx.x] = (uint32_t)(c0 ^ c1 ^ c2 ^ c3 ^ c4 ^ c5 ^ c6 ^ c7) ^ h0 ^ h1 ^ h2 ^ h3;
}

// ------------------------------------------------------------------------------------------------ host side
// Every extern "C" entry takes the context's (recursive) lock: a context may be shared between threads, calls are serialised.
// Host-buffer entries stage through grow-only device buffers and two streams that the context owns (no allocation or stream
// creation per call once the sizes have been seen); device-pointer entries only enqueue, and order their use of the
// workspace against earlier calls on other streams with an event.
#define MBLS_N_STAGE 11
// measured crossovers (scripts/throughput_vs_n.py, 128 keys, device-resident): one wave per item wins up to ~5 k items (10.3 ms at 4 096, ~11.8 at
// 5 120); the lane path with four lanes per item in the Miller loop and two in the message phase and the final exponentiation (products in pairs)
// needs 12.2-12.7 ms for anything up to a quarter of a round
#define MBLS_DEFAULT_COOP_MAX_ITEMS 5120
#define MBLS_DEFAULT_COOP_HASH_MAX_ITEMS 3584           /* above n / 4 + 2 n / 64 > 1 024 waves: the four-per-wave message phase needs a second round beside the key sums and the signatures (3 600 items 8.0 ms, 3 648 items 9.9 ms); the lane-pair form takes 8.8 - 9.0 */
#define MBLS_DEFAULT_TRACKS_MIN_REST 3584
struct mbls_ctx {
    std::recursive_mutex mu;
    int device = 0;
    uint64_t cap = 0;                  // items the workspace can hold
    uint32_t* d_w = nullptr;           // workspace limbs
    uint32_t* d_status = nullptr;      // per-item status (when the caller passes none)
    uint8_t* d_results = nullptr;
    uint32_t* d_scalar = nullptr;      // small scratch words
    uint32_t* d_gtab = nullptr;        // [64 * 16][MBLS_KEYREC_DWORDS]: [d 16^j] G1 (sk -> pk), built on first use
    uint32_t* d_skidx = nullptr; uint64_t skidx_cap = 0;      // the table indices of a batch of secret keys
    uint32_t* d_sksel = nullptr; uint64_t sksel_cap = 0;      // constant-time sk -> pk: the records each (key, window) selected, [chunk * 64][MBLS_KEYREC_DWORDS]
    bool secret_ops_fast = false;      // false (default): table lookups that depend on a secret key are scans with selection (mbls_ctx_set_secret_ops)
    uint64_t key_cap = 0;              // decompressed-key staging (compressed wire format): capacity in keys
    uint32_t* d_keys_xy = nullptr;     // [key_cap][24] affine Montgomery coordinates
    uint8_t* d_key_flags = nullptr;
    // shared message lists (mbls_*_shared_msgs): the hashed points of a call's list, [72][htab_cap] dwords (entry 0: H of the empty message, hashed on the first
    // call after every (re)allocation; message j: entry j + 1), one bad-range word per entry, and the status words of the list's own hash
    uint64_t htab_cap = 0; uint32_t* d_htab = nullptr; uint32_t* d_hflag = nullptr; uint32_t* d_hst = nullptr; bool h_empty_ready = false;
    // verify_multiple over a shared list, grouped by message (mbls_vms.h): per table entry the sets that name it, the cursor that hands out their positions and
    // the exclusive scan, and over a resident table (mbls_vmt.h) the named flags, their scan and the named entries (d_hgrp: [MBLS_HGRP_ARRAYS][hgrp_cap], sized by
    // reserve_groups for the list or the table of the call), and per workspace item the map position -> message (d_vmap: [cap], with the workspace)
    uint32_t* d_hgrp = nullptr; uint64_t hgrp_cap = 0; uint32_t* d_vmap = nullptr;
    int vm_grouping = 0;               // mbls_ctx_set_vm_grouping: 0 auto (vms_grouped), 1 always one Miller loop per message, 2 never
    struct { void* p; size_t cap; } stage[MBLS_N_STAGE] = {};
    hipStream_t hs_a = nullptr, hs_b = nullptr, hs_c = nullptr, hs_d = nullptr;      // streams of the host-buffer entry points (hs_d: the signature phase while hs_b uploads keys)
    hipEvent_t hs_ev = nullptr, hs_ev2 = nullptr, hs_ev3 = nullptr;
    // the second TRACK of the verification pipeline (verify_pipeline): a batch between one and two rounds runs as two halves side by side, each with its own part
    // of the workspace, its own main stream and its own side streams for the front phases
    hipStream_t t1_s = nullptr, t1_b = nullptr, t1_c = nullptr;
    hipEvent_t t1_ev = nullptr, t1_ev2 = nullptr, t1_ev3 = nullptr;
    hipEvent_t ws_ev = nullptr; hipStream_t ws_stream = nullptr; bool ws_pending = false;   // last asynchronous user of the workspace
    bool timing = false;
    hipEvent_t ev[MBLS_N_PHASES + 1] = {};
    float phase_ms[MBLS_N_PHASES] = {};
    std::vector<struct mbls_keytable*> tables;     // the key tables created on this context (orphaned when it is destroyed)
    std::vector<struct mbls_msgtable*> msgtables;  // the message tables, likewise
    std::vector<struct mbls_committees*> committees;   // the committee tables, likewise
    // committee entries (mbls_cmt.h): the items' index lists k_cmt_expand writes for k_aggregate_cmt_d -- cmt_words uint32 in all, an item's list at a stride of the
    // table's largest committee -- and the count and route words of cmt_items items (d_cmt_cnt: [2][cmt_items]); mbls_ctx_reserve_committee_items
    uint32_t* d_cmt_list = nullptr; uint64_t cmt_words = 0; uint32_t* d_cmt_cnt = nullptr; uint64_t cmt_items = 0;
    int cmt_route_mode = 0;            // mbls_ctx_set_committee_route: 0 auto (cmt_route), 1 always direct, 2 complement whenever eligible
    int vm_span_split = 0;             // mbls_ctx_set_vm_span_split: 0 auto (mbls_vcs.h vcs_split), else the split factor 1, 2, 4, 8 or 16
    // committee spans (mbls_cms.h): the items' list regions k_cms_expand writes for k_aggregate_cms_d -- cms_words uint32 in all, an item's region at the stride of
    // the call (cms_stride) --, and for cms_items items the records (d_cms_rec: [cms_items][MBLS_CMS_REC_DWORDS]) and the parked points (d_cms_park:
    // [MBLS_CMS_PARK_DWORDS][cms_items]); mbls_ctx_reserve_committee_span_items
    uint32_t* d_cms_list = nullptr; uint64_t cms_words = 0; uint32_t* d_cms_rec = nullptr; uint32_t* d_cms_park = nullptr; uint64_t cms_items = 0;
    coop_prog coop[10] = {};           // the cooperative engine's microprograms in HBM (mbls_coop.h): pairing2, vmtail, f12mul, g2add, smiller, vmfinal, hashg2, miller1,
                                       // pairing2x2 (two items per wave), hashg2x4 (four)
    uint32_t* d_coop = nullptr; size_t coop_bytes = 0;
    // measured crossovers (scripts/coop_sweep.py, 128 keys, device-resident): one wave per item for the pairing check wins up to ~10 k items
    // (19.7 ms at 10 240 against 22.5), for the message phase as well up to ~6 k (13.3 ms at 6 144 against 14.0; four items per wave above 768)
    uint64_t coop_hash_max_items = MBLS_DEFAULT_COOP_HASH_MAX_ITEMS;
    uint64_t coop_max_items = MBLS_DEFAULT_COOP_MAX_ITEMS;
    // within (pack_min, pack_max] a wave serves two items (pairing check) / four items (message phase) side by side: more steps per wave, fewer per item
    uint64_t coop_pack_min_items = 1024, coop_pack_max_items = 2048, coop_hash_pack_min_items = 768;
    // one ROUND of the one-lane kernels = one wave on every SIMD (512 registers per lane: one wave per SIMD) = CUs x 4 x 64 items. A batch of
    // q rounds + r items would cost q + 1 rounds of every kernel; the r items are cut off and take the route of an r-item batch instead
    uint64_t round_items = 65536;
    // batches of at most split_max_items items (default: half a round) on the one-lane path walk their two Miller pairs on two lanes (k_miller_split);
    // up to fork_max_items items the three front phases (keys | signature | message) run side by side on the context's streams
    uint64_t split_max_items = 32768, fork_max_items = 49152, hash2_max_items = 20480;
    // a batch of one to two rounds whose remainder over the round is at least tracks_min_rest items runs as two equal halves on two tracks (0: never)
    uint64_t tracks_min_rest = MBLS_DEFAULT_TRACKS_MIN_REST;
    uint64_t tracks_side_max = 16384;  // remainders up to this many items run BESIDE the last round (a track of their own) instead of as one of two equal halves
    char err[256] = {};
};
struct mbls_keytable {
    mbls_ctx* c = nullptr;             // nullptr: the context was destroyed first (the records went with it)
    uint32_t* d_recs = nullptr;        // [cap][MBLS_KEYREC_DWORDS]
    uint64_t size = 0, cap = 0;
    hipEvent_t ev = nullptr; hipStream_t ev_stream = nullptr; bool pending = false;   // the last asynchronous append
};
// resident message table (mbls_mtb.h): [72][stride] dwords and one flag word per entry, stride = cap + 1 (entry 0: H of the empty message, hashed at creation;
// public index j: entry j + 1); d_st: the status words of the appends' own hashes, by entry
struct mbls_msgtable {
    mbls_ctx* c = nullptr;             // nullptr: the context was destroyed first
    uint32_t* d_tab = nullptr; uint32_t* d_flag = nullptr; uint32_t* d_st = nullptr;
    uint64_t size = 0, cap = 0;
    hipEvent_t ev = nullptr; hipStream_t ev_stream = nullptr; bool pending = false;   // the last asynchronous append
    std::atomic<long long> stream_calls{0};        // calls of streams bound to the table that have not completed (mbls_msgtable_clear refuses while there are any)
};
// committee table (mbls_cmt.h): the member lists back to back (key-table indices) and one record per committee
struct mbls_committees {
    mbls_ctx* c = nullptr;             // nullptr: the context was destroyed first
    mbls_keytable* kt = nullptr;       // the key table the members index
    uint32_t* d_members = nullptr; uint64_t n_members = 0, members_cap = 0;
    uint32_t* d_recs = nullptr; uint64_t count = 0, cap = 0;      // [cap][MBLS_CMT_REC_DWORDS]
    uint32_t max_members = 0;          // the largest committee the table holds
    std::vector<uint32_t> sizes;       // every committee's member count, by id: what the host entries of the span form check an item's field against
    hipEvent_t ev = nullptr; hipStream_t ev_stream = nullptr; bool pending = false;   // the last asynchronous append
    std::atomic<long long> stream_calls{0};        // calls of streams bound to the table that have not completed (mbls_committees_clear refuses while there are any)
    std::vector<uint64_t> stream_bits;             // 8 * bits_stride of every stream bound to the table: mbls_committees_append keeps every committee inside the smallest
};
typedef std::lock_guard<std::recursive_mutex> mbls_lock;

#define HIPCHK(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    snprintf((ctx)->err, sizeof((ctx)->err), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); return MBLS_ERR_DEVICE; } } while (0)
#define ARGFAIL(ctx, what) do { snprintf((ctx)->err, sizeof((ctx)->err), "invalid argument: %s", what); return MBLS_ERR_ARGUMENT; } while (0)

static inline unsigned nblk(uint64_t n) { return (unsigned)((n + WG - 1) / WG); }
// the message phase of n items on stream s: one lane per item (k_hash), or -- small batches -- hash_to_field per lane and the rest one wave per item
// pair_ok: the caller's workspace view holds 2 n items and nothing else uses slots 7..24 / 31..42 of items [0, 2 n) meanwhile -- batches of at most
// half a round then take two lanes per message (k_hash2)
enum { HASH_FORM_AUTO = 0, HASH_FORM_LANE, HASH_FORM_WAVE, HASH_FORM_PAIR };
static void launch_hash(mbls_ctx* c, mbls_ws ws, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff, uint32_t* st, uint64_t n, hipStream_t s, bool pair_ok = false,
                        int form = HASH_FORM_AUTO);
// the per-item key sum from wire-format keys: the generated routine for 96-byte keys (its 16-byte loads want 4-byte alignment),
// the compiled lane body for 48-byte keys summed in place and for unaligned buffers
static void launch_aggregate(mbls_ws ws, const uint8_t* d_pks, const uint32_t* d_off, uint32_t k, int fmt, int mode, uint32_t* st, uint64_t n, hipStream_t s) {
    if (fmt == MBLS_PK_UNCOMPRESSED && (((uintptr_t)d_pks) & 3u) == 0)
        hipLaunchKernelGGL(k_aggregate_raw_d, dim3(nblk(n)), dim3(WG), 0, s, ws, d_pks, d_off, k, mode, st, n);
    else
        hipLaunchKernelGGL(k_aggregate, dim3(nblk(n)), dim3(WG), 0, s, ws, d_pks, d_off, k, fmt, mode, st, n);
}

// one launch of the cooperative kernel: program `prog` on n_items items (64 / lpi of them per wave)
enum { COOP_PAIRING2 = 0, COOP_VMTAIL, COOP_F12MUL, COOP_G2ADD, COOP_SMILLER, COOP_VMFINAL, COOP_HASHG2, COOP_MILLER1, COOP_PAIRING2X2, COOP_HASHG2X4 };
static void coop_run(mbls_ctx* c, int prog, mbls_ws ws, uint64_t first_item, uint64_t item_step, uint64_t partner_step, uint64_t n_items, uint32_t* st, uint8_t* res,
                     int res_mode, hipStream_t s, const uint32_t* d_live = nullptr) {
    const coop_prog& pg = c->coop[prog];
    const uint64_t ipw = 64 / pg.lpi;
    const dim3 grid((unsigned)((n_items + ipw - 1) / ipw));
    const size_t lds = COOP_LDS_BYTES(pg);
    if (prog == COOP_HASHG2X4)
        hipLaunchKernelGGL(k_coop_pow_x4, grid, dim3(64), lds, s, pg, ws, first_item, item_step, partner_step, n_items, st, res, res_mode, d_live);
    else if (prog == COOP_HASHG2)
        hipLaunchKernelGGL(k_coop_pow, grid, dim3(64), lds, s, pg, ws, first_item, item_step, partner_step, n_items, st, res, res_mode, d_live);
    else if (prog == COOP_PAIRING2X2)
        hipLaunchKernelGGL(k_coop_x2, grid, dim3(64), lds, s, pg, ws, first_item, item_step, partner_step, n_items, st, res, res_mode, d_live);
    else
        hipLaunchKernelGGL(k_coop, grid, dim3(64), lds, s, pg, ws, first_item, item_step, partner_step, n_items, st, res, res_mode, d_live);
}
// which form the message phase of n items takes: lane pairs (k_hash2) where the caller reserved 2 n workspace items and the batch is above the wave engine's range
// but at most hash2_max_items (5/16 of a round: 2 n lanes for the messages beside n for the keys, with the signatures behind them, are still resident together; at a
// third of a round and above the doubled message phase pushes the key sums behind it: 20 480 items 16.1 -> 14.6 ms, 21 845 items 16.3 -> 16.7); one wave per item
// (or four items per wave) up to coop_hash_max_items -- the measured crossover, for every caller --; one lane per item otherwise
static int hash_form(const mbls_ctx* c, uint64_t n, bool pair_ok, bool no_waves = false) {
    const bool waves = !no_waves && n <= c->coop_hash_max_items && n <= c->coop_max_items;
    if (pair_ok && !waves && n <= c->split_max_items && n <= c->hash2_max_items) return HASH_FORM_PAIR;
    return waves ? HASH_FORM_WAVE : HASH_FORM_LANE;
}
static void launch_hash(mbls_ctx* c, mbls_ws ws, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff, uint32_t* st, uint64_t n, hipStream_t s, bool pair_ok, int form) {
    if (form == HASH_FORM_AUTO) form = hash_form(c, n, pair_ok);
    if (form == HASH_FORM_PAIR) {
        hipLaunchKernelGGL(k_hash2, dim3(nblk(2 * n)), dim3(WG), 0, s, ws, d_msgs, msg_len, d_moff, st, n);
        hipLaunchKernelGGL(k_h_compact_a, dim3(nblk(n)), dim3(WG), 0, s, ws, n);
        hipLaunchKernelGGL(k_h_compact_b, dim3(nblk(n)), dim3(WG), 0, s, ws, n);
    } else if (form == HASH_FORM_WAVE) {
        hipLaunchKernelGGL(k_hash_fields, dim3(nblk(n)), dim3(WG), 0, s, ws, d_msgs, msg_len, d_moff, st, n);
        coop_run(c, n > c->coop_hash_pack_min_items ? COOP_HASHG2X4 : COOP_HASHG2, ws, (uint64_t)0, (uint64_t)1, (uint64_t)0, n, (uint32_t*)nullptr, (uint8_t*)nullptr, COOP_RES_ITEM, s);
    } else
        hipLaunchKernelGGL(k_hash, dim3(nblk(n)), dim3(WG), 0, s, ws, d_msgs, msg_len, d_moff, st, n);
}
static void ctx_free(mbls_ctx* c) {
    (void)hipSetDevice(c->device);
    if (c->d_w) (void)hipFree(c->d_w);
    if (c->d_status) (void)hipFree(c->d_status);
    if (c->d_results) (void)hipFree(c->d_results);
    if (c->d_scalar) (void)hipFree(c->d_scalar);
    if (c->d_gtab) (void)hipFree(c->d_gtab);
    if (c->d_skidx) (void)hipFree(c->d_skidx);
    if (c->d_sksel) (void)hipFree(c->d_sksel);
    if (c->d_keys_xy) (void)hipFree(c->d_keys_xy);
    if (c->d_key_flags) (void)hipFree(c->d_key_flags);
    if (c->d_htab) (void)hipFree(c->d_htab);
    if (c->d_hflag) (void)hipFree(c->d_hflag);
    if (c->d_hst) (void)hipFree(c->d_hst);
    if (c->d_hgrp) (void)hipFree(c->d_hgrp);
    if (c->d_vmap) (void)hipFree(c->d_vmap);
    if (c->d_cmt_list) (void)hipFree(c->d_cmt_list);
    if (c->d_cmt_cnt) (void)hipFree(c->d_cmt_cnt);
    if (c->d_cms_list) (void)hipFree(c->d_cms_list);
    if (c->d_cms_rec) (void)hipFree(c->d_cms_rec);
    if (c->d_cms_park) (void)hipFree(c->d_cms_park);
    if (c->d_coop) (void)hipFree(c->d_coop);
    for (int i = 0; i < MBLS_N_STAGE; i++) if (c->stage[i].p) (void)hipFree(c->stage[i].p);
    for (int i = 0; i <= MBLS_N_PHASES; i++) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    if (c->hs_ev) (void)hipEventDestroy(c->hs_ev);
    if (c->hs_ev2) (void)hipEventDestroy(c->hs_ev2);
    if (c->hs_ev3) (void)hipEventDestroy(c->hs_ev3);
    if (c->t1_ev) (void)hipEventDestroy(c->t1_ev);
    if (c->t1_ev2) (void)hipEventDestroy(c->t1_ev2);
    if (c->t1_ev3) (void)hipEventDestroy(c->t1_ev3);
    if (c->t1_s) (void)hipStreamDestroy(c->t1_s);
    if (c->t1_b) (void)hipStreamDestroy(c->t1_b);
    if (c->t1_c) (void)hipStreamDestroy(c->t1_c);
    if (c->ws_ev) (void)hipEventDestroy(c->ws_ev);
    if (c->hs_a) (void)hipStreamDestroy(c->hs_a);
    if (c->hs_b) (void)hipStreamDestroy(c->hs_b);
    if (c->hs_c) (void)hipStreamDestroy(c->hs_c);
    if (c->hs_d) (void)hipStreamDestroy(c->hs_d);
    delete c;
}
static void ctx_default_tuning(mbls_ctx* c);
extern "C" int mbls_ctx_create(mbls_ctx** out, int device_id) {
    if (!out) return MBLS_ERR_ARGUMENT;
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0 || device_id < 0 || device_id >= cnt) return MBLS_ERR_DEVICE;
    if (hipSetDevice(device_id) != hipSuccess) return MBLS_ERR_DEVICE;
    mbls_ctx* c = new (std::nothrow) mbls_ctx();
    if (!c) return MBLS_ERR_DEVICE;
    c->device = device_id;
    bool ok = true;
    for (int i = 0; i <= MBLS_N_PHASES; i++) ok = ok && hipEventCreate(&c->ev[i]) == hipSuccess;
    ok = ok && hipMalloc(&c->d_scalar, 64) == hipSuccess;
    // the side streams of the front phases: when the three chains do not fit the chip side by side (above a quarter of a round), the message phase -- the
    // longest of them -- is to get its SIMDs first and the signature phase -- the shortest -- last (32 768 items: the front takes 4.4 ms instead of 5.0)
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);           // (numerically: lowest priority, highest priority)
    if (getenv("MBLS_NO_STREAM_PRIORITIES")) prio_lo = prio_hi = 0;
    ok = ok && hipStreamCreateWithFlags(&c->hs_a, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithPriority(&c->hs_b, hipStreamNonBlocking, prio_lo) == hipSuccess &&
         hipStreamCreateWithPriority(&c->hs_c, hipStreamNonBlocking, prio_hi) == hipSuccess && hipStreamCreateWithPriority(&c->hs_d, hipStreamNonBlocking, prio_lo) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->hs_ev, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&c->hs_ev2, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&c->hs_ev3, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&c->ws_ev, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&c->t1_s, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithPriority(&c->t1_b, hipStreamNonBlocking, prio_lo) == hipSuccess &&
         hipStreamCreateWithPriority(&c->t1_c, hipStreamNonBlocking, prio_hi) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->t1_ev, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&c->t1_ev2, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&c->t1_ev3, hipEventDisableTiming) == hipSuccess;
    if (ok) {       // the cooperative engine's programs: one upload per context
#define COOP_SRC(P) {MBLS_COOP_##P##_STEPS, MBLS_COOP_##P##_ROWS, MBLS_COOP_##P##_CONSTS}
#define COOP_CNT(P) {2 * MBLS_COOP_##P##_NSTEPS, 512 * MBLS_COOP_##P##_NROWS, 15 * (MBLS_COOP_##P##_NCONSTS ? MBLS_COOP_##P##_NCONSTS : 1)}
        const int NP = 10;
        const uint32_t* src[NP][3] = {COOP_SRC(PAIRING2), COOP_SRC(VMTAIL), COOP_SRC(F12MUL), COOP_SRC(G2ADD), COOP_SRC(SMILLER), COOP_SRC(VMFINAL), COOP_SRC(HASHG2),
                                      COOP_SRC(MILLER1), COOP_SRC(PAIRING2X2), COOP_SRC(HASHG2X4)};
        const size_t cnt[NP][3] = {COOP_CNT(PAIRING2), COOP_CNT(VMTAIL), COOP_CNT(F12MUL), COOP_CNT(G2ADD), COOP_CNT(SMILLER), COOP_CNT(VMFINAL), COOP_CNT(HASHG2),
                                   COOP_CNT(MILLER1), COOP_CNT(PAIRING2X2), COOP_CNT(HASHG2X4)};
        const uint32_t nconst[NP] = {MBLS_COOP_PAIRING2_NCONSTS, MBLS_COOP_VMTAIL_NCONSTS, MBLS_COOP_F12MUL_NCONSTS, MBLS_COOP_G2ADD_NCONSTS, MBLS_COOP_SMILLER_NCONSTS,
                                     MBLS_COOP_VMFINAL_NCONSTS, MBLS_COOP_HASHG2_NCONSTS, MBLS_COOP_MILLER1_NCONSTS, MBLS_COOP_PAIRING2X2_NCONSTS, MBLS_COOP_HASHG2X4_NCONSTS};
#define COOP_DIM(P) {MBLS_COOP_##P##_LPI, MBLS_COOP_##P##_NSLOTS}
        const uint32_t dims[NP][2] = {COOP_DIM(PAIRING2), COOP_DIM(VMTAIL), COOP_DIM(F12MUL), COOP_DIM(G2ADD), COOP_DIM(SMILLER), COOP_DIM(VMFINAL), COOP_DIM(HASHG2),
                                      COOP_DIM(MILLER1), COOP_DIM(PAIRING2X2), COOP_DIM(HASHG2X4)};
        size_t total = 0;
        for (int p = 0; p < NP; p++) for (int a = 0; a < 3; a++) total += (cnt[p][a] + 3) & ~(size_t)3;       // 16-byte aligned pieces (the rows are read as uint4)
        ok = hipMalloc(&c->d_coop, total * 4) == hipSuccess; c->coop_bytes = ok ? total * 4 : 0;
        size_t at = 0;
        for (int p = 0; p < NP && ok; p++) {
            const uint32_t* dp[3];
            for (int a = 0; a < 3 && ok; a++) {
                dp[a] = c->d_coop + at;
                ok = hipMemcpy(c->d_coop + at, src[p][a], cnt[p][a] * 4, hipMemcpyHostToDevice) == hipSuccess;
                at += (cnt[p][a] + 3) & ~(size_t)3;
            }
            c->coop[p].steps = dp[0]; c->coop[p].rows = dp[1]; c->coop[p].consts = dp[2]; c->coop[p].nconsts = nconst[p];
            c->coop[p].lpi = dims[p][0]; c->coop[p].nslots = dims[p][1];
        }
        ctx_default_tuning(c);
    }
    if (!ok) { ctx_free(c); return MBLS_ERR_DEVICE; }
    *out = c; return MBLS_OK;
}
// batches of up to max_items items run their pairing check one wave per item (mbls_coop.h); 0 = always one lane per item
extern "C" int mbls_ctx_set_coop_max_items(mbls_ctx* c, uint64_t max_items) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu); c->coop_max_items = max_items; return MBLS_OK;
}
extern "C" int mbls_ctx_set_coop_hash_max_items(mbls_ctx* c, uint64_t max_items) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu); c->coop_hash_max_items = max_items; return MBLS_OK;
}
extern "C" int mbls_ctx_set_coop_packing(mbls_ctx* c, uint64_t pairing_min_items, uint64_t pairing_max_items, uint64_t hash_min_items) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu); c->coop_pack_min_items = pairing_min_items; c->coop_pack_max_items = pairing_max_items; c->coop_hash_pack_min_items = hash_min_items; return MBLS_OK;
}
// every routing parameter back to its default (what mbls_ctx_create sets, environment included)
static void ctx_default_tuning(mbls_ctx* c) {
    c->vm_grouping = 0; c->cmt_route_mode = 0; c->vm_span_split = 0;
    c->coop_max_items = MBLS_DEFAULT_COOP_MAX_ITEMS; c->coop_hash_max_items = MBLS_DEFAULT_COOP_HASH_MAX_ITEMS;
    c->coop_pack_min_items = 1024; c->coop_pack_max_items = 2048; c->coop_hash_pack_min_items = 768;
    hipDeviceProp_t prop;
    c->round_items = 65536;
    if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) c->round_items = (uint64_t)prop.multiProcessorCount * 4 * WG;
    c->split_max_items = c->round_items / 2; c->fork_max_items = c->round_items / 4 * 3; c->hash2_max_items = c->round_items / 16 * 5;
    const char* e;
    if ((e = getenv("MBLS_COOP_MAX_ITEMS"))) c->coop_max_items = strtoull(e, nullptr, 10);
    if ((e = getenv("MBLS_COOP_HASH_MAX_ITEMS"))) c->coop_hash_max_items = strtoull(e, nullptr, 10);
    if ((e = getenv("MBLS_SPLIT_MAX_ITEMS"))) c->split_max_items = strtoull(e, nullptr, 10);
    if ((e = getenv("MBLS_FORK_MAX_ITEMS"))) c->fork_max_items = strtoull(e, nullptr, 10);
    if ((e = getenv("MBLS_HASH2_MAX_ITEMS"))) c->hash2_max_items = strtoull(e, nullptr, 10);
    c->secret_ops_fast = getenv("MBLS_UNSAFE_SECRET_OPS") != nullptr;
    c->tracks_min_rest = MBLS_DEFAULT_TRACKS_MIN_REST; c->tracks_side_max = c->round_items / 4;
    if ((e = getenv("MBLS_TRACKS_MIN_REST"))) c->tracks_min_rest = strtoull(e, nullptr, 10);
    if ((e = getenv("MBLS_TRACKS_SIDE_MAX"))) c->tracks_side_max = strtoull(e, nullptr, 10);
}
extern "C" int mbls_ctx_reset_tuning(mbls_ctx* c) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    ctx_default_tuning(c); return MBLS_OK;
}
// verify_multiple over a shared message list: 0 auto (group when 2 n_msgs <= n), 1 always one Miller loop per message, 2 never (mbls_vms.h vms_grouped)
extern "C" int mbls_ctx_set_vm_grouping(mbls_ctx* c, int mode) {
    if (!c || mode < 0 || mode > 2) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    c->vm_grouping = mode; return MBLS_OK;
}
// committee entries: 0 auto (complement when eligible and (m - s) + 1 < s, mbls_cmt.h cmt_route), 1 always direct, 2 complement whenever eligible
extern "C" int mbls_ctx_set_committee_route(mbls_ctx* c, int mode) {
    if (!c || mode < 0 || mode > 2) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    c->cmt_route_mode = mode; return MBLS_OK;
}
// verify_multiple over committee spans: 0 auto (mbls_vcs.h vcs_split), else the lanes each of a set's two key lists is cut over: 1, 2, 4, 8 or 16
extern "C" int mbls_ctx_set_vm_span_split(mbls_ctx* c, int mode) {
    if (!c || !vcs_split_mode_ok(mode)) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    c->vm_span_split = mode; return MBLS_OK;
}
extern "C" int mbls_plan_committee_route(uint32_t m, uint32_t s, int eligible, int mode) {
    if (mode < 0 || mode > 2 || m == 0 || m > MBLS_CMT_MAX_MEMBERS || s > m) return MBLS_ERR_ARGUMENT;
    return cmt_route(m, s, eligible != 0, mode);
}
// items per round of the one-lane kernels (default: CUs x 4 SIMDs x 64 lanes); batches above it have their remainder routed as a batch of its own
extern "C" int mbls_ctx_set_round_items(mbls_ctx* c, uint64_t items) {
    if (!c || (items && items % WG)) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (!items) {
        hipDeviceProp_t prop;
        HIPCHK(c, hipGetDeviceProperties(&prop, c->device));
        items = (uint64_t)prop.multiProcessorCount * 4 * WG;
    }
    c->round_items = items; c->split_max_items = items / 2; c->fork_max_items = items / 4 * 3; c->hash2_max_items = items / 16 * 5; c->tracks_side_max = items / 4; return MBLS_OK;
}
// one-lane path: batches of up to split_max_items items walk their two Miller pairs on two lanes (never above half a round); up to
// fork_max_items items the three front phases run side by side. Defaults: round / 2 and 3/4 of a round (measured: side by side costs 26.6 ms
// at 57 344 items and 30.2 at 65 535, in a row 26.1 and 26.4; at 32 768 it is 17.1 against 19.3); 0 = never.
extern "C" int mbls_ctx_set_lane_shaping(mbls_ctx* c, uint64_t split_max_items, uint64_t fork_max_items) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    c->split_max_items = split_max_items > c->round_items / 2 ? c->round_items / 2 : split_max_items;
    c->fork_max_items = fork_max_items; return MBLS_OK;
}
extern "C" void mbls_ctx_destroy(mbls_ctx* c) {
    if (!c) return;
    {
        mbls_lock lk(c->mu); (void)hipSetDevice(c->device); (void)hipDeviceSynchronize();
        for (mbls_keytable* t : c->tables) {      // tables that outlive their context become empty shells: mbls_keytable_destroy only frees the handle
            if (t->d_recs) (void)hipFree(t->d_recs);
            if (t->ev) (void)hipEventDestroy(t->ev);
            t->d_recs = nullptr; t->ev = nullptr; t->size = t->cap = 0; t->c = nullptr;
        }
        c->tables.clear();
        for (mbls_msgtable* t : c->msgtables) {
            if (t->d_tab) (void)hipFree(t->d_tab);
            if (t->d_flag) (void)hipFree(t->d_flag);
            if (t->d_st) (void)hipFree(t->d_st);
            if (t->ev) (void)hipEventDestroy(t->ev);
            t->d_tab = t->d_flag = t->d_st = nullptr; t->ev = nullptr; t->size = t->cap = 0; t->c = nullptr;
        }
        c->msgtables.clear();
        for (mbls_committees* t : c->committees) {
            if (t->d_members) (void)hipFree(t->d_members);
            if (t->d_recs) (void)hipFree(t->d_recs);
            if (t->ev) (void)hipEventDestroy(t->ev);
            t->d_members = t->d_recs = nullptr; t->ev = nullptr; t->count = t->cap = t->n_members = t->members_cap = 0; t->max_members = 0; t->kt = nullptr; t->c = nullptr;
        }
        c->committees.clear();
    }
    ctx_free(c);
}
extern "C" const char* mbls_last_error(mbls_ctx* c) { return c ? c->err : "null context"; }
extern "C" int mbls_ctx_reserve(mbls_ctx* c, uint64_t max_items) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t want = ((max_items + 1 + WG - 1) / WG) * WG;     // +1: the extra (sig, -G1) lane of the n-pairing paths
    if (want <= c->cap) return MBLS_OK;
    if (c->d_w) { (void)hipFree(c->d_w); (void)hipFree(c->d_status); (void)hipFree(c->d_results); c->d_w = nullptr; c->d_status = nullptr; c->d_results = nullptr; c->cap = 0; }
    if (c->d_vmap) { (void)hipFree(c->d_vmap); c->d_vmap = nullptr; }
    HIPCHK(c, hipMalloc(&c->d_w, (size_t)MBLS_SLOT_TOTAL * 12 * want * 4));
    HIPCHK(c, hipMalloc(&c->d_vmap, want * 4));
    HIPCHK(c, hipMalloc(&c->d_status, want * 4));
    HIPCHK(c, hipMalloc(&c->d_results, want));
    c->cap = want; return MBLS_OK;
}
// staging for decompressed keys (compressed wire format with a uniform key count)
static int reserve_keys(mbls_ctx* c, uint64_t nkeys) {
    if (nkeys <= c->key_cap) return MBLS_OK;
    if (c->d_keys_xy) { (void)hipFree(c->d_keys_xy); (void)hipFree(c->d_key_flags); c->d_keys_xy = nullptr; c->d_key_flags = nullptr; c->key_cap = 0; }
    HIPCHK(c, hipMalloc(&c->d_keys_xy, nkeys * 96));
    HIPCHK(c, hipMalloc(&c->d_key_flags, nkeys));
    c->key_cap = nkeys; return MBLS_OK;
}
extern "C" int mbls_ctx_reserve_keys(mbls_ctx* c, uint64_t max_keys) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return reserve_keys(c, max_keys);
}
// the group arrays of verify_multiple's grouped route alone, for `entries` messages of a list or entries of a resident table (+ 1: the scans' last word): a call
// over a resident table needs these and no call table (288 bytes per entry that it would never read). Grow-only; growth drains the device like mbls_ctx_reserve.
#define MBLS_HGRP_ARRAYS 6                    /* cnt, cur, off (mbls_vms.h); flag, roff, named (mbls_vmt.h) */
static int reserve_groups(mbls_ctx* c, uint64_t entries) {
    const uint64_t want = ((entries + 1 + WG - 1) / WG) * WG;
    if (want <= c->hgrp_cap) return MBLS_OK;
    if (c->d_hgrp) { (void)hipFree(c->d_hgrp); c->d_hgrp = nullptr; c->hgrp_cap = 0; }
    HIPCHK(c, hipMalloc(&c->d_hgrp, (size_t)MBLS_HGRP_ARRAYS * want * 4));
    c->hgrp_cap = want; return MBLS_OK;
}
// the table of hashed points of a shared message list: max_msgs messages + the entry of the empty message (grow-only; growth drains the device like mbls_ctx_reserve)
static int reserve_msgs(mbls_ctx* c, uint64_t max_msgs) {
    const int rg = reserve_groups(c, max_msgs); if (rg) return rg;
    const uint64_t want = ((max_msgs + 1 + WG - 1) / WG) * WG;
    if (want <= c->htab_cap) return MBLS_OK;
    if (c->d_htab) { (void)hipFree(c->d_htab); (void)hipFree(c->d_hflag); (void)hipFree(c->d_hst); c->d_htab = nullptr; c->d_hflag = nullptr; c->d_hst = nullptr; c->htab_cap = 0; }
    c->h_empty_ready = false;
    HIPCHK(c, hipMalloc(&c->d_htab, (size_t)MBLS_H_DWORDS * want * 4));
    HIPCHK(c, hipMalloc(&c->d_hflag, want * 4));
    HIPCHK(c, hipMalloc(&c->d_hst, want * 4));
    c->htab_cap = want; return MBLS_OK;
}
extern "C" int mbls_ctx_reserve_msgs(mbls_ctx* c, uint64_t max_msgs) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return reserve_msgs(c, max_msgs);
}
extern "C" int mbls_enable_phase_timing(mbls_ctx* c, int on) { if (!c) return MBLS_ERR_ARGUMENT; mbls_lock lk(c->mu); c->timing = on != 0; return MBLS_OK; }
extern "C" int mbls_last_phase_ms(mbls_ctx* c, float ms[MBLS_N_PHASES]) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    for (int i = 0; i < MBLS_N_PHASES; i++) ms[i] = c->phase_ms[i];
    return MBLS_OK;
}

// a view of one of the context's grow-only staging buffers (host-buffer entry points; the lock makes the reuse safe)
struct sbuf {
    mbls_ctx* c; int slot; void* p = nullptr;
    sbuf(mbls_ctx* c_, int slot_) : c(c_), slot(slot_) {}
    hipError_t alloc(size_t bytes) {
        if (!bytes) bytes = 1;
        auto& s = c->stage[slot];
        if (s.cap < bytes) {
            if (s.p) { (void)hipFree(s.p); s.p = nullptr; s.cap = 0; }
            size_t want = bytes < 4096 ? 4096 : bytes + bytes / 8;
            hipError_t e = hipMalloc(&s.p, want); if (e != hipSuccess) return e;
            s.cap = want;
        }
        p = s.p; return hipSuccess;
    }
    hipError_t up(const void* h, size_t bytes) { hipError_t e = alloc(bytes); if (e != hipSuccess || !bytes) return e; return hipMemcpy(p, h, bytes, hipMemcpyHostToDevice); }
    hipError_t down(void* h, size_t bytes) { return bytes ? hipMemcpy(h, p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
    template <typename T> T* as() { return (T*)p; }
};

// cross-stream ordering of the shared workspace: a call on stream s first waits for the last asynchronous user on another stream
static int ws_acquire(mbls_ctx* c, hipStream_t s) {
    if (c->ws_pending && c->ws_stream != s) HIPCHK(c, hipStreamWaitEvent(s, c->ws_ev, 0));
    return MBLS_OK;
}
static int ws_release(mbls_ctx* c, hipStream_t s) {
    HIPCHK(c, hipEventRecord(c->ws_ev, s)); c->ws_stream = s; c->ws_pending = true; return MBLS_OK;
}

// readers of a key table on stream s wait (on the device) for the last asynchronous append made on another stream
static int table_acquire(mbls_ctx* c, const mbls_keytable* t, hipStream_t s) {
    if (t && t->pending && t->ev_stream != s) HIPCHK(c, hipStreamWaitEvent(s, t->ev, 0));
    return MBLS_OK;
}
static int msgtable_acquire(mbls_ctx* c, const mbls_msgtable* t, hipStream_t s) {
    if (t->pending && t->ev_stream != s) HIPCHK(c, hipStreamWaitEvent(s, t->ev, 0));
    return MBLS_OK;
}
static int committees_acquire(mbls_ctx* c, const mbls_committees* t, hipStream_t s) {
    if (t && t->pending && t->ev_stream != s) HIPCHK(c, hipStreamWaitEvent(s, t->ev, 0));
    return MBLS_OK;
}
// the scratch of the committee entries for `items` items of up to `members` members each (grow-only; growth frees and allocates, which drains the device)
static int reserve_committee(mbls_ctx* c, uint64_t items, uint64_t members) {
    if (!members) members = 1;
    const uint64_t want_items = ((items + WG - 1) / WG) * WG, want_words = want_items * members;
    if (want_items > c->cmt_items) {
        if (c->d_cmt_cnt) { (void)hipFree(c->d_cmt_cnt); c->d_cmt_cnt = nullptr; c->cmt_items = 0; }
        HIPCHK(c, hipMalloc(&c->d_cmt_cnt, want_items * 2 * 4));
        c->cmt_items = want_items;
    }
    if (want_words > c->cmt_words) {
        if (c->d_cmt_list) { (void)hipFree(c->d_cmt_list); c->d_cmt_list = nullptr; c->cmt_words = 0; }
        HIPCHK(c, hipMalloc(&c->d_cmt_list, want_words * 4));
        c->cmt_words = want_words;
    }
    return MBLS_OK;
}
extern "C" int mbls_ctx_reserve_committee_items(mbls_ctx* c, uint64_t max_items, uint32_t max_members) {
    if (!c || max_members > MBLS_CMT_MAX_MEMBERS) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return reserve_committee(c, max_items, max_members);
}
// the scratch of the span entries for `items` items whose list regions take `stride` words each (grow-only, like reserve_committee)
static int reserve_committee_span(mbls_ctx* c, uint64_t items, uint64_t stride) {
    if (!stride) stride = 1;
    const uint64_t want_items = ((items + WG - 1) / WG) * WG, want_words = want_items * stride;
    if (want_items > c->cms_items) {
        if (c->d_cms_rec) { (void)hipFree(c->d_cms_rec); c->d_cms_rec = nullptr; }
        if (c->d_cms_park) { (void)hipFree(c->d_cms_park); c->d_cms_park = nullptr; }
        c->cms_items = 0;
        HIPCHK(c, hipMalloc(&c->d_cms_rec, want_items * MBLS_CMS_REC_DWORDS * 4));
        HIPCHK(c, hipMalloc(&c->d_cms_park, want_items * MBLS_CMS_PARK_DWORDS * 4));
        c->cms_items = want_items;
    }
    if (want_words > c->cms_words) {
        if (c->d_cms_list) { (void)hipFree(c->d_cms_list); c->d_cms_list = nullptr; c->cms_words = 0; }
        HIPCHK(c, hipMalloc(&c->d_cms_list, want_words * 4));
        c->cms_words = want_words;
    }
    return MBLS_OK;
}
extern "C" int mbls_ctx_reserve_committee_span_items(mbls_ctx* c, uint64_t max_items, uint32_t max_item_members) {
    if (!c || max_item_members > MBLS_CMS_MAX_COMMITTEES * MBLS_CMT_MAX_MEMBERS) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return reserve_committee_span(c, max_items, max_item_members);
}
extern "C" int mbls_plan_committee_span(const uint32_t* sizes, const uint8_t* eligible, uint32_t q, const uint8_t* bits, uint32_t bits_bytes, int mode,
                                        uint64_t* complement_mask, uint32_t* n_direct_listed, uint32_t* n_missing_listed) {
    if (!complement_mask || !n_direct_listed || !n_missing_listed || (q && (!sizes || !eligible)) || (bits_bytes && !bits)) return MBLS_ERR_ARGUMENT;
    return cms_plan_item(sizes, eligible, q, bits, bits_bytes, mode, complement_mask, n_direct_listed, n_missing_listed) ? MBLS_ERR_ARGUMENT : MBLS_OK;
}
// the key source of an _indexed entry: the table at the size it has now (the caller holds the context's lock)
static int keys_of_table(mbls_ctx* c, const mbls_keytable* t, const uint32_t* d_idx, const uint32_t* d_off, keysrc* ks) {
    if (t->c != c) ARGFAIL(c, "key table belongs to another context");
    *ks = keys_table(t->d_recs, t->size, d_idx, d_off, t); return MBLS_OK;
}
// the key source of a _committee entry (defined with the committee table below), and what a host entry hands verify_host beside it: ids and bitfields in host memory
static int keys_of_committees(mbls_ctx* c, const mbls_committees* t, const uint32_t* d_cmt_idx, const uint8_t* d_bits, uint32_t bits_stride, bool device_bits, keysrc* ks);
// (the span form: cmt_idx null, item i names ids cmt_ids[cmt_off[i] .. cmt_off[i + 1]) of n_cmt_ids)
struct host_committees {
    const mbls_committees* t; const uint32_t* cmt_idx; const uint8_t* bits; uint32_t bits_stride;
    bool span = false; const uint32_t* cmt_ids = nullptr; uint64_t n_cmt_ids = 0; const uint32_t* cmt_off = nullptr;
};
static int keys_of_committee_span(mbls_ctx* c, const mbls_committees* t, const uint32_t* d_cmt_ids, uint64_t n_cmt_ids, const uint32_t* d_cmt_off, const uint8_t* d_bits,
                                  uint32_t bits_stride, bool device_bits, keysrc* ks);
static int committee_span_items_ok(mbls_ctx* c, const host_committees& hc, uint64_t n);
// The message source of a _msgtable entry. The entry hands over the indices alone (msgs_in_table): what the table holds lives in its handle until verify_device /
// verify_host, under the context's lock and once they know the table is this context's, read it at the size it has then (msgs_of_table).
static msgsrc msgs_in_table(const uint32_t* d_idx) { return msgs_table(nullptr, 0, nullptr, 0, d_idx); }
static msgsrc msgs_of_table(const mbls_msgtable* t, const uint32_t* d_idx) { return msgs_table(t->d_tab, mtb_stride(t->cap), t->d_flag, t->size, d_idx); }

// ---- routing as data (include/mbls.h, mbls_plan_batch): the decisions of the verification pipeline as pure functions of the limits and the batch size. The
// pipeline below acts on exactly these structures, so what mbls_plan_batch reports is what runs.
static mbls_limits ctx_limits(const mbls_ctx* c) {
    mbls_limits L;
    L.round_items = c->round_items; L.coop_max_items = c->coop_max_items; L.coop_hash_max_items = c->coop_hash_max_items;
    L.coop_pack_min_items = c->coop_pack_min_items; L.coop_pack_max_items = c->coop_pack_max_items; L.coop_hash_pack_min_items = c->coop_hash_pack_min_items;
    L.split_max_items = c->split_max_items; L.fork_max_items = c->fork_max_items; L.hash2_max_items = c->hash2_max_items;
    L.tracks_min_rest = c->tracks_min_rest; L.tracks_side_max = c->tracks_side_max;
    return L;
}
extern "C" void mbls_default_limits(uint64_t round_items, mbls_limits* out) {
    if (!out) return;
    if (!round_items) round_items = 65536;
    out->round_items = round_items; out->coop_max_items = MBLS_DEFAULT_COOP_MAX_ITEMS; out->coop_hash_max_items = MBLS_DEFAULT_COOP_HASH_MAX_ITEMS;
    out->coop_pack_min_items = 1024; out->coop_pack_max_items = 2048; out->coop_hash_pack_min_items = 768;
    out->split_max_items = round_items / 2; out->fork_max_items = round_items / 4 * 3; out->hash2_max_items = round_items / 16 * 5;
    out->tracks_min_rest = MBLS_DEFAULT_TRACKS_MIN_REST; out->tracks_side_max = round_items / 4;
}
// one pass over n items. no_waves: the pass stays on the lane kernels (a remainder beside a round); fork_max: front phases side by side up to this many items
// (~0: the limits' own); keys_later: the host entries' two-part form (their signature phase always has a stream of its own)
static void plan_pass(const mbls_limits& L, uint64_t n, bool no_waves, uint64_t fork_max, bool keys_later, bool timing, mbls_pass_plan* p) {
    const uint64_t coop_max = no_waves ? 0 : L.coop_max_items, coop_hash_max = no_waves ? 0 : L.coop_hash_max_items;
    const bool split = n > coop_max && n <= L.split_max_items && 2 * n <= L.round_items;       // two lanes per item in the Miller phase
    // (a batch whose pairing check runs on waves but whose message phase does not takes the lane-pair message phase too: 2 n items of workspace)
    const bool hash_pairs = split || (n <= coop_max && n > coop_hash_max && n <= L.split_max_items && 4 * n <= L.round_items);
    p->items = n; p->workspace_items = hash_pairs ? 2 * n : n;
    if (n <= coop_max) p->pairing = (n > L.coop_pack_min_items && n <= L.coop_pack_max_items) ? MBLS_PAIRING_WAVE_X2 : MBLS_PAIRING_WAVE;
    else if (split) p->pairing = 4 * n <= L.round_items ? MBLS_PAIRING_LANES4 : MBLS_PAIRING_LANES2;
    else p->pairing = MBLS_PAIRING_LANE;
    // the message phase: lane pairs (k_hash2) where 2 n workspace items are there and the batch is above the wave engine's range but at most hash2_max_items (5/16 of
    // a round: 2 n lanes for the messages beside n for the keys, with the signatures behind them, are still resident together; at a third of a round and above the
    // doubled message phase pushes the key sums behind it: 20 480 items 16.1 -> 14.6 ms, 21 845 items 16.3 -> 16.7); one wave per item (four items per wave above the
    // packing limit) up to coop_hash_max_items -- the measured crossover, for every caller --; one lane per item otherwise
    const bool waves = n <= coop_hash_max && n <= coop_max;
    if (hash_pairs && !waves && n <= L.split_max_items && n <= L.hash2_max_items) p->message = MBLS_MESSAGE_LANES2;
    else if (waves) p->message = n > L.coop_hash_pack_min_items ? MBLS_MESSAGE_WAVE_X4 : MBLS_MESSAGE_WAVE;
    else p->message = MBLS_MESSAGE_LANE;
    p->sig_subgroup_from_miller_loop = n > coop_max ? 1u : 0u;     // one lane (or lane pairs) per item: the signature's subgroup test comes out of the Miller loop
    const bool fork = !timing && n <= (fork_max == ~0ull ? L.fork_max_items : fork_max);
    // above a quarter of a round the three chains no longer fit the chip side by side (and the message phase runs on n lanes, its longest form): the signature
    // phase -- the shortest -- then follows the key sum on the caller's stream, beside the message phase: 32 768 items 17.1 -> 16.5 ms
    const bool sig_side = fork && (keys_later || 4 * n <= L.round_items);
    p->front = !fork ? MBLS_FRONT_IN_A_ROW : sig_side ? MBLS_FRONT_ALL_BESIDE : MBLS_FRONT_MESSAGE_BESIDE;
}
// The batch as the caller sees it. n = q rounds + r items (0 < r < round): a batch of q rounds + r items would cost q + 1 rounds of every kernel, so
//   r < tracks_min_rest: the q rounds as one launch per kernel, then the r items as a batch of their own that takes the route of its size (wave engine up to coop_max_items);
//   r >= tracks_min_rest: the q - 1 rounds in front, then the LAST round and the remainder on TWO TRACKS side by side, each with its own part of the workspace and its
//   own streams, so that the SIMDs one leaves idle take waves of the other -- up to tracks_side_max (and a quarter of a round) the round on track 0 and the remainder,
//   on the lane-pair forms whatever its size, on track 1 (69 120 ... 76 000 items 33.7 ms against 34.5 ... 40 in a row; scripts/dbg/rest_probe.py, rest_probe2.py),
//   above it two equal halves of (R + r) / 2 items (100 000 items 51.6 -> 46.5 ms; scripts/dbg/tracks_probe.py).
// (The phase timers describe a single pass: no cut while they are on -- the caller passes one_pass.)
static void plan_batch(const mbls_limits& L, uint64_t n, bool one_pass, bool timing, mbls_batch_plan* b) {
    memset(b, 0, sizeof(*b));
    const uint64_t R = L.round_items;
    auto pass = [&](int i, uint64_t first, uint64_t items, uint32_t stage, uint32_t trk, uint64_t ws_first, bool no_waves, uint64_t fork_max) {
        plan_pass(L, items, no_waves, fork_max, false, timing, &b->pass[i]);
        b->pass[i].first_item = first; b->pass[i].stage = stage; b->pass[i].track = trk; b->pass[i].workspace_first = ws_first;
    };
    if (one_pass || !R || n <= R || n % R == 0) { b->mode = MBLS_BATCH_ONE_PASS; b->n_passes = 1; pass(0, 0, n, 0, 0, 0, false, ~0ull); return; }
    const uint64_t r = n % R;
    const bool two = L.tracks_min_rest && r >= L.tracks_min_rest && (R + r) / 2 > L.split_max_items && (R + r) / 2 > L.coop_max_items;   // (halves take one workspace item per item)
    if (!two) {
        b->mode = MBLS_BATCH_ROUNDS_THEN_REST; b->n_passes = 2;
        pass(0, 0, n - r, 0, 0, 0, false, ~0ull); pass(1, n - r, r, 1, 0, 0, false, ~0ull);
        return;
    }
    const bool side = r <= L.tracks_side_max && 4 * r <= R;
    const uint64_t lo = n - r - R;                                   // the whole rounds in front: one launch per kernel
    const uint64_t half = side ? R : ((R + r) / 2 + WG - 1) / WG * WG;   // items [lo, lo + half) on track 0, the rest on track 1 (cut at a bitmap word)
    int i = 0; uint32_t stage = 0;
    if (lo) { pass(i++, 0, lo, stage++, 0, 0, false, ~0ull); }
    b->mode = side ? MBLS_BATCH_ROUND_BESIDE_REST : MBLS_BATCH_TWO_HALVES;
    // the halves' front phases side by side only while a half is at most 19/32 of a round and no round runs in front (scripts/dbg/tracks_probe.py: r = 6 144 ... 10 240
    // 36.7 against 37.7 ms; r = 18 432 ... 30 720 in a row 38.0 ... 40.1 against 38.8 ... 42.0; behind a round 64.4 against 67.1 at r = 10 240 ... 20 480); in side
    // mode each part follows the rule of its own size
    const uint64_t fm = side ? ~0ull : ((lo == 0 && half <= R / 32 * 19) ? L.fork_max_items : 0);
    pass(i++, lo, half, stage, 0, 0, false, fm);
    pass(i++, lo + half, n - lo - half, stage, 1, half, side, fm);
    b->n_passes = (uint32_t)i;
}
extern "C" int mbls_plan_batch(const mbls_limits* limits, uint64_t n, mbls_batch_plan* out) {
    if (!limits || !out || !n) return MBLS_ERR_ARGUMENT;
    plan_batch(*limits, n, false, false, out); return MBLS_OK;
}
// the workspace items the plan of n items needs when every item has k keys in a layout that allows the eight-lane key sum (see pass_key_split): what
// verify_pipeline reserves before it queues the first pass -- mbls_ctx_reserve(ctx, this) beforehand keeps every allocation out of the call
extern "C" uint64_t mbls_plan_workspace_items(const mbls_limits* limits, uint64_t n, uint32_t k, int split_layout) {
    if (!limits || !n) return 0;
    mbls_batch_plan bp; plan_batch(*limits, n, false, false, &bp);
    uint64_t need = 0;
    for (uint32_t i = 0; i < bp.n_passes; i++) {
        const mbls_pass_plan& pp = bp.pass[i];
        const bool on_waves = pp.pairing == MBLS_PAIRING_WAVE || pp.pairing == MBLS_PAIRING_WAVE_X2;
        const bool ksplit = split_layout && on_waves && k >= 4 * MBLS_KEY_SPLIT && k % MBLS_KEY_SPLIT == 0;
        const uint64_t w = ksplit && pp.items * (1 + MBLS_KEY_SPLIT) > pp.workspace_items ? pp.items * (1 + MBLS_KEY_SPLIT) : pp.workspace_items;
        if (pp.workspace_first + w > need) need = pp.workspace_first + w;
    }
    return need;
}
// Shared message lists (mbls_*_shared_msgs): the plan of the n items is plan_batch's with every pass's message phase a gather from the context's table of hashed
// points, and the list of n_msgs messages is hashed by launch_hash in the form ITS size asks for -- the forms and limits of plan_pass's message phase, applied to the
// messages of one piece: the wave engine up to coop_hash_max_items (four per wave above the packing limit), lane pairs (2 workspace items per message) up to
// hash2_max_items and half a round, one lane per message otherwise. A piece is at most one round of messages (more would cost a second round of k_hash anyway, and
// the workspace a call reserves for its list stays at one round); message j of a piece works in workspace item j of the call's workspace.
static void plan_shared(const mbls_limits& L, uint64_t n, uint64_t n_msgs, bool one_pass, bool timing, mbls_shared_msgs_plan* sp) {
    memset(sp, 0, sizeof(*sp));
    plan_batch(L, n, one_pass, timing, &sp->batch);
    for (uint32_t i = 0; i < sp->batch.n_passes; i++) sp->batch.pass[i].message = MBLS_MESSAGE_GATHER;
    sp->table_entries = n_msgs + 1;
    if (!n_msgs) return;
    const uint64_t R = L.round_items;
    const uint64_t m = (R && n_msgs > R) ? R : n_msgs;               // messages of a (full) piece
    const bool waves = m <= L.coop_hash_max_items && m <= L.coop_max_items;
    const bool pairs = !waves && m <= L.split_max_items && m <= L.hash2_max_items && 2 * m <= R;
    sp->list_message = waves ? (m > L.coop_hash_pack_min_items ? MBLS_MESSAGE_WAVE_X4 : MBLS_MESSAGE_WAVE) : pairs ? MBLS_MESSAGE_LANES2 : MBLS_MESSAGE_LANE;
    sp->list_piece_items = m;
    sp->list_pieces = (n_msgs + m - 1) / m;
    sp->list_workspace_items = pairs ? 2 * m : m;
}
extern "C" int mbls_plan_batch_shared_msgs(const mbls_limits* limits, uint64_t n, uint64_t n_msgs, mbls_shared_msgs_plan* out) {
    if (!limits || !out || !n) return MBLS_ERR_ARGUMENT;
    plan_shared(*limits, n, n_msgs, false, false, out); return MBLS_OK;
}
// what a shared-message call reserves before it queues anything: the larger of the items' plan (mbls_plan_workspace_items) and the list hash's items
extern "C" uint64_t mbls_plan_shared_msgs_workspace_items(const mbls_limits* limits, uint64_t n, uint64_t n_msgs, uint32_t k, int split_layout) {
    if (!limits || !n) return 0;
    mbls_shared_msgs_plan sp; plan_shared(*limits, n, n_msgs, false, false, &sp);
    const uint64_t a = mbls_plan_workspace_items(limits, n, k, split_layout);
    return a > sp.list_workspace_items ? a : sp.list_workspace_items;
}
// verify_multiple over a shared message list (mbls_verify_multiple*_shared_msgs): the route, the form of the list hash (plan_shared's), the Miller items, the
// tree levels and the workspace, as a pure function of the limits -- what verify_multiple_impl acts on. The thresholds are verify_multiple_impl's: n for the
// per-set chains, the Miller items for the Miller phase.
static void plan_vm_shared(const mbls_limits& L, uint64_t n, uint64_t n_msgs, int mode, uint64_t longest, mbls_vm_shared_msgs_plan* vp) {
    memset(vp, 0, sizeof(*vp));
    mbls_shared_msgs_plan sp; plan_shared(L, n, n_msgs, false, false, &sp);
    vp->list_message = sp.list_message; vp->list_pieces = sp.list_pieces; vp->list_piece_items = sp.list_piece_items;
    vp->list_workspace_items = sp.list_workspace_items; vp->table_entries = sp.table_entries;
    const bool grouped = vms_grouped(n, n_msgs, mode);
    vp->route = grouped ? MBLS_VM_ROUTE_GROUPED : MBLS_VM_ROUTE_PER_SET;
    vp->miller_items = grouped ? vms_miller_items(n_msgs) : n;
    vp->tree_levels = grouped ? vms_levels(n, longest) : 0;
    vp->workspace_items = vms_workspace_items(n, n_msgs, grouped, sp.list_workspace_items);
    vp->chains_beside = 2 * n <= L.round_items ? 1 : 0;
    vp->sig_lane_pairs = 2 * n <= L.coop_max_items ? 1 : 0;
    const uint64_t m = vp->miller_items, R = L.round_items;
    if (2 * m <= L.coop_max_items) { vp->miller = MBLS_PAIRING_WAVE; vp->miller_rest_items = m; }       // npairing_finish / launch_miller_single
    else {
        const uint64_t full = (R && m > R) ? (m / R) * R : 0, rest = m - full;
        vp->miller_rounds = R ? full / R : 0; vp->miller_rest_items = rest;
        vp->miller = (rest && 2 * rest <= R) ? MBLS_PAIRING_LANES2 : MBLS_PAIRING_LANE;
    }
}
extern "C" int mbls_plan_verify_multiple_shared_msgs(const mbls_limits* limits, uint64_t n, uint64_t n_msgs, int mode, mbls_vm_shared_msgs_plan* out) {
    if (!limits || !out || !n || mode < 0 || mode > 2) return MBLS_ERR_ARGUMENT;
    plan_vm_shared(*limits, n, n_msgs, mode, 0, out); return MBLS_OK;
}
extern "C" uint64_t mbls_plan_verify_multiple_shared_msgs_workspace_items(const mbls_limits* limits, uint64_t n, uint64_t n_msgs, int mode) {
    if (!limits || !n || mode < 0 || mode > 2) return 0;
    mbls_vm_shared_msgs_plan vp; plan_vm_shared(*limits, n, n_msgs, mode, 0, &vp);
    return vp.workspace_items;
}
// verify_multiple over the resident message table (mbls_verify_multiple*_msgtable*): plan_vm_shared's rule with `bound` -- what the host knows about the number
// of distinct entries the call names (mbls_vmt.h vmt_bound) -- in place of the list length, and no list: nothing is hashed, no call table is needed
static void plan_vm_msgtable(const mbls_limits& L, uint64_t n, uint64_t table_size, uint64_t named, int mode, uint64_t longest, mbls_vm_shared_msgs_plan* vp) {
    plan_vm_shared(L, n, vmt_bound(n, table_size, named), mode, longest, vp);
    vp->list_message = 0; vp->list_pieces = 0; vp->list_piece_items = 0; vp->list_workspace_items = 0; vp->table_entries = 0;
    vp->workspace_items = vmt_workspace_items(n, vmt_bound(n, table_size, named), vp->route == MBLS_VM_ROUTE_GROUPED);
}
extern "C" int mbls_plan_verify_multiple_msgtable(const mbls_limits* limits, uint64_t n, uint64_t table_size, uint64_t named, int mode, mbls_vm_shared_msgs_plan* out) {
    if (!limits || !out || !n || mode < 0 || mode > 2) return MBLS_ERR_ARGUMENT;
    plan_vm_msgtable(*limits, n, table_size, named, mode, 0, out); return MBLS_OK;
}
extern "C" uint64_t mbls_plan_verify_multiple_msgtable_workspace_items(const mbls_limits* limits, uint64_t n, uint64_t table_size, uint64_t named, int mode) {
    if (!limits || !n || mode < 0 || mode > 2) return 0;
    mbls_vm_shared_msgs_plan vp; plan_vm_msgtable(*limits, n, table_size, named, mode, 0, &vp);
    return vp.workspace_items;
}
extern "C" uint64_t mbls_plan_verify_multiple_msgtable_locate_workspace_items(const mbls_limits* limits, uint64_t n, uint64_t table_size, uint64_t named, int mode) {
    if (!limits || !n || mode < 0 || mode > 2) return 0;
    mbls_vm_shared_msgs_plan vp; plan_vm_msgtable(*limits, n, table_size, named, mode, 0, &vp);
    return vsl_workspace_items(n, vmt_bound(n, table_size, named), vp.route == MBLS_VM_ROUTE_GROUPED, 0);
}
// verify_multiple over committee spans (mbls_verify_multiple_committee_span_msgtable*): the split factor of the key phase (mbls_vcs.h vcs_split) and what the call
// reserves -- the message-table entries' figure plus the partial sums' items (vcs_extra_items: 2 P n under a split, none without)
extern "C" int mbls_plan_verify_multiple_span(const mbls_limits* limits, uint64_t n, uint64_t table_size, uint64_t stride_words, int locate, int split_mode,
                                                        uint32_t* split, uint64_t* workspace_items) {
    if (!limits || !n || !split || !workspace_items || !vcs_split_mode_ok(split_mode)) return MBLS_ERR_ARGUMENT;
    const uint32_t P = vcs_split(n, stride_words ? stride_words : 1, limits, split_mode);
    mbls_vm_shared_msgs_plan vp; plan_vm_msgtable(*limits, n, table_size, 0, 0, 0, &vp);
    const uint64_t w = locate ? vsl_workspace_items(n, vmt_bound(n, table_size, 0), vp.route == MBLS_VM_ROUTE_GROUPED, 0) : vp.workspace_items;
    *split = P; *workspace_items = w + vcs_extra_items(n, P);
    return MBLS_OK;
}
#ifdef MBLS_COOP_PROFILE
extern "C" int mbls_coop_profile_read(unsigned long long out[64], int reset) {     // dev builds only (not declared in mbls.h)
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mbls_coop_prof), 64 * 8) != hipSuccess) return MBLS_ERR_DEVICE;
    if (reset) { unsigned long long z[64] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(mbls_coop_prof), z, 64 * 8) != hipSuccess) return MBLS_ERR_DEVICE; }
    return MBLS_OK;
}
#endif
extern "C" int mbls_ctx_get_limits(mbls_ctx* c, mbls_limits* out) {
    if (!c || !out) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu); *out = ctx_limits(c); return MBLS_OK;
}
// A TRACK = what one pass of the pipeline owns besides the caller's stream: where its items start in the workspace (and in the status words / key staging that go
// with it), the side streams of its front phases and the events that join them. Track 0 is the context's own set; verify_pipeline runs a second one beside it.
struct track {
    uint64_t ws_off = 0;
    hipStream_t sb = nullptr, sc = nullptr, sd = nullptr;
    hipEvent_t ev2 = nullptr, ev3 = nullptr;
    bool ws_sync = true;              // order the pass against the workspace's previous user and record its own end (false: the caller does both around its tracks)
    uint64_t fork_max = ~0ull;        // front phases side by side up to this many items (~0: the context's fork_max_items)
    bool no_waves = false;            // the pass stays on the lane kernels whatever its size (a remainder BESIDE a round: the wave engine's 40 KB-of-LDS waves would wait
                                      // for SIMDs the round's 512-register waves hold, and its latency advantage is worth nothing next to a 26 ms round)
};
// The eight-lane key sum of a pass on the wave engine (see verify_pipeline_one) and the workspace items the pass then needs: n items + 8 n partial sums. Both are
// functions of the pass plan, the key source and the keys per item -- verify_pipeline sizes the workspace of a whole plan with them BEFORE the first pass is queued.
static bool pass_key_split(const mbls_pass_plan& pp, const keysrc& ks, uint32_t k) {
    const bool on_waves = pp.pairing == MBLS_PAIRING_WAVE || pp.pairing == MBLS_PAIRING_WAVE_X2;
    const bool staged = !ks.indexed && ks.fmt == MBLS_PK_COMPRESSED && !ks.d_off && k > 1;
    return on_waves && !staged && !ks.committee && !ks.d_off && k >= 4 * MBLS_KEY_SPLIT && k % MBLS_KEY_SPLIT == 0 &&
           (ks.indexed || (ks.fmt == MBLS_PK_UNCOMPRESSED && (((uintptr_t)ks.d_pks) & 3u) == 0));
}
static uint64_t pass_ws_items(const mbls_pass_plan& pp, const keysrc& ks, uint32_t k, uint64_t n) {
    const uint64_t split = pass_key_split(pp, ks, k) ? n + n * MBLS_KEY_SPLIT : 0;
    return split > pp.workspace_items ? split : pp.workspace_items;
}
// where the points of a hashed list go: the context's per-call table, or a resident table behind the entries it already holds
struct htab_dst { uint32_t* tab; uint64_t tstride; uint32_t* flags; uint32_t* st; uint64_t first_entry; };
// the hash of the list on stream s: piece after piece through launch_hash in workspace items [0, piece), each followed by its export to the table; first of all,
// once per allocation of the table, the entry of the empty message
static int shared_hash_list(mbls_ctx* c, const mbls_shared_msgs_plan& sp, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff, uint64_t n_msgs, hipStream_t s,
                            const htab_dst* dst = nullptr) {
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    const htab_dst own = {c->d_htab, c->htab_cap, c->d_hflag, c->d_hst, 1};
    const htab_dst& d = dst ? *dst : own;
    if (!dst && !c->h_empty_ready) {
        HIPCHK(c, hipMemsetAsync(c->d_hst, 0, 4, s));
        launch_hash(c, ws, (const uint8_t*)c->d_htab, 0u, (const uint64_t*)nullptr, c->d_hst, (uint64_t)1, s);
        hipLaunchKernelGGL(k_h_export_tab, dim3(1), dim3(MBLS_HB), 0, s, ws, c->d_htab, c->htab_cap, c->d_hflag, (const uint32_t*)c->d_hst, (uint64_t)0, (uint64_t)1);
        c->h_empty_ready = true;
    }
    const int form = sp.list_message == MBLS_MESSAGE_LANE ? HASH_FORM_LANE : sp.list_message == MBLS_MESSAGE_LANES2 ? HASH_FORM_PAIR : HASH_FORM_WAVE;
    for (uint64_t first = 0; first < n_msgs; first += sp.list_piece_items) {
        const uint64_t m = n_msgs - first < sp.list_piece_items ? n_msgs - first : sp.list_piece_items;
        uint32_t* st_list = d.st + d.first_entry + first;
        HIPCHK(c, hipMemsetAsync(st_list, 0, 4 * m, s));
        // uniform messages advance the base pointer, an offset table is absolute (its slice goes with the unmoved base)
        launch_hash(c, ws, (d_moff || !d_msgs) ? d_msgs : d_msgs + (uint64_t)msg_len * first, msg_len, d_moff ? d_moff + first : nullptr, st_list, m, s,
                    form == HASH_FORM_PAIR, form);
        hipLaunchKernelGGL(k_h_export_tab, dim3((unsigned)((m + MBLS_HB - 1) / MBLS_HB)), dim3(MBLS_HB), 0, s, ws, d.tab, d.tstride, d.flags, (const uint32_t*)st_list,
                           d.first_entry + first, m);
    }
    HIPCHK(c, hipGetLastError());
    return MBLS_OK;
}
static track track0(mbls_ctx* c) { track t; t.sb = c->hs_b; t.sc = c->hs_c; t.sd = c->hs_d; t.ev2 = c->hs_ev2; t.ev3 = c->hs_ev3; return t; }
static int verify_pipeline_one(mbls_ctx* c, const batch& b, hipStream_t s, int part = 0, const track* tkp = nullptr, bool no_growth = false) {
    const keysrc& ks = b.ks; const msgsrc& ms = b.ms;
    const uint8_t* const d_sigs = b.d_sigs; uint8_t* const d_results = b.d_results; uint64_t* const d_bitmap = b.d_bitmap; uint32_t* const d_status = b.d_status;
    const uint64_t n = b.n; const uint32_t k = b.k; const int mode = b.mode;
    const int fmt = ks.fmt; const uint32_t* d_off = ks.d_off;
    if (!c || (fmt != MBLS_PK_COMPRESSED && fmt != MBLS_PK_UNCOMPRESSED)) return MBLS_ERR_ARGUMENT;
    if (n == 0) return MBLS_OK;
    const bool have_keys = ks.span ? (ks.d_cmt_span_off != nullptr && (ks.d_cmt_ids != nullptr || !ks.n_cmt_ids) && (ks.d_bits != nullptr || !ks.bits_stride))
                         : ks.committee ? (ks.d_cmt_idx != nullptr && ks.d_bits != nullptr) : ks.indexed ? (ks.d_idx != nullptr) : (ks.d_pks != nullptr);
    if (!d_sigs || (!ms.indexed() && !ms.d_msgs && ms.msg_len && !ms.d_moff) || (ms.indexed() && !ms.d_idx) || !d_results || (!have_keys && (k || d_off) && part != 1))
        ARGFAIL(c, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    const track tk = tkp ? *tkp : track0(c);
    bool tm = c->timing;
    // what this pass does is decided by plan_pass (the function mbls_plan_batch reports from): forms of the pairing check and of the message phase, workspace, forks
    mbls_pass_plan pp; plan_pass(ctx_limits(c), n, tk.no_waves, tk.fork_max, part != 0, tm, &pp);
    const bool on_waves = pp.pairing == MBLS_PAIRING_WAVE || pp.pairing == MBLS_PAIRING_WAVE_X2;
    const bool split = pp.pairing == MBLS_PAIRING_LANES2 || pp.pairing == MBLS_PAIRING_LANES4;     // lane pairs / quads in the Miller phase, pairs in the final exponentiation
    const bool hash_pairs = pp.workspace_items == 2 * n;
    const int hform = pp.message == MBLS_MESSAGE_LANE ? HASH_FORM_LANE : pp.message == MBLS_MESSAGE_LANES2 ? HASH_FORM_PAIR : HASH_FORM_WAVE;
    bool staged = !ks.indexed && (fmt == MBLS_PK_COMPRESSED) && !d_off && k > 1;   // lane-per-key decompression, then the per-item sums
    // batches on the wave engine are latency: the key sum of 128 keys is a 2 ms chain on one lane -- eight lanes take an eighth of the keys each (items of k / 8
    // keys lie back to back just like that) and k_apk_combine adds their sums: 0.4 ms
    // (pass_key_split: the same predicate verify_pipeline sizes the workspace of a several-pass plan with -- a pass that is not the first of its call finds its
    // space reserved and never grows the workspace under a pass in flight: `no_growth` passes that would not fit fall back to the one-lane key sum)
    bool key_split = pass_key_split(pp, ks, k);
    if (key_split && no_growth && tk.ws_off + pass_ws_items(pp, ks, k, n) > c->cap) key_split = false;
    const uint64_t nsub = key_split ? n * MBLS_KEY_SPLIT : 0;
    const uint64_t ws_items = key_split && n + nsub > pp.workspace_items ? n + nsub : pp.workspace_items;
    if (no_growth && tk.ws_off + ws_items > c->cap) ARGFAIL(c, "internal: a later pass of a plan would have to grow the workspace");
    int rc = mbls_ctx_reserve(c, tk.ws_off + ws_items); if (rc) return rc;        // (a pass on a second track finds its space reserved: no growth under the first)
    mbls_ws ws; ws.w = c->d_w + tk.ws_off; ws.stride = c->cap;
    uint32_t* st = d_status ? d_status : c->d_status + tk.ws_off;
    unsigned g = nblk(n);
    if (staged) { rc = reserve_keys(c, (tk.ws_off + n) * (uint64_t)k); if (rc) return rc; }
    uint32_t* const keys_xy = staged ? c->d_keys_xy + 24 * (uint64_t)k * tk.ws_off : nullptr;
    uint8_t* const key_flags = staged ? c->d_key_flags + (uint64_t)k * tk.ws_off : nullptr;
    // The status words are zeroed and every phase ORs its bits in (atomically), so the three phases before the Miller loop can run in
    // any order -- and, for batches that leave most SIMDs idle (n <= 2^14: at most a quarter of the one-wave-per-SIMD slots), side by
    // side on the context's own streams: keys | signature | message, joined before the Miller loop (latency 35.7 -> ~30 ms).
    // part 1 / part 2 (host-buffer entry points): the signature and message phases are queued first (part 1, the keys may be
    // null), the caller then uploads the keys on another stream and makes this one wait, and part 2 queues the rest.
    const bool keys_later = part != 0;
    const bool fused_sig = pp.sig_subgroup_from_miller_loop != 0;     // the subgroup test of the signature comes out of the Miller loop, k_sig only decodes
    const bool fork = pp.front != MBLS_FRONT_IN_A_ROW;
    // (host-buffer entries: hs_b carries the key upload, so their signature phase has a stream of its own)
    const bool sig_side = pp.front == MBLS_FRONT_ALL_BESIDE;
    hipStream_t s_sig = sig_side ? (part == 0 ? tk.sb : tk.sd) : s, s_msg = fork ? tk.sc : s;
    if (part != 2) {
        if (tk.ws_sync) { rc = ws_acquire(c, s); if (rc) return rc; }
        HIPCHK(c, hipMemsetAsync(st, 0, 4 * n, s));
        if (fork) {
            HIPCHK(c, hipEventRecord(tk.ev2, s));
            if (s_sig != s) HIPCHK(c, hipStreamWaitEvent(s_sig, tk.ev2, 0));
            HIPCHK(c, hipStreamWaitEvent(s_msg, tk.ev2, 0));
        }
    }
    // batches on the wave engine are latency: their signature chain (decode + subgroup ladder, 2.1 ms on one lane) is the longest of the three front chains --
    // two lanes per signature there (k_sig2: 1.6 ms)
    auto launch_sig = [&]() {
        if (on_waves && !fused_sig) hipLaunchKernelGGL(k_sig2, dim3(nblk(2 * n)), dim3(WG), 0, s_sig, ws, d_sigs, st, n);
        else hipLaunchKernelGGL(k_sig, dim3(g), dim3(WG), 0, s_sig, ws, d_sigs, st, n, fused_sig ? 0 : 1);
    };
    // the message phase: the items' own messages through launch_hash, or -- a shared list -- [the hash of the list and its export, then] the gather from the table
    auto launch_msg = [&]() -> int {
        if (!ms.indexed()) { launch_hash(c, ws, ms.d_msgs, ms.msg_len, ms.d_moff, st, n, s_msg, hash_pairs, hform); return MBLS_OK; }
        if (ms.list) { const int rl = shared_hash_list(c, *ms.list, ms.d_msgs, ms.msg_len, ms.d_moff, ms.n_msgs, s_msg); if (rl) return rl; }
        hipLaunchKernelGGL(k_h_gather, dim3((unsigned)((n + MBLS_HB - 1) / MBLS_HB)), dim3(MBLS_HB), 0, s_msg, ws, ms.tab, ms.tstride, ms.flags, ms.d_idx, ms.n_msgs, st, n);
        return MBLS_OK;
    };
    if (part == 1) {
        launch_sig();
        rc = launch_msg(); if (rc) return rc;
        HIPCHK(c, hipGetLastError());
        return MBLS_OK;
    }
    if (tm) HIPCHK(c, hipEventRecord(c->ev[0], s));
    if (ks.indexed) { rc = table_acquire(c, ks.tab, s); if (rc) return rc; }
    if (ks.span) {
        // the items' list regions, records and parked points in the span scratch reserved for the whole plan (reserve_committee_span), at the pass's workspace offset
        const uint64_t ls = cms_stride(ks.bits_stride, ks.cmax);
        if ((tk.ws_off + n) * ls > c->cms_words || tk.ws_off + n > c->cms_items) ARGFAIL(c, "internal: the span scratch of a pass was not reserved");
        rc = committees_acquire(c, ks.cmt, s); if (rc) return rc;
        uint32_t* const list = c->d_cms_list + tk.ws_off * ls; uint32_t* const irec = c->d_cms_rec + tk.ws_off * MBLS_CMS_REC_DWORDS;
        mbls_cms_launch_expand(ks.d_crecs, ks.ccount, ks.d_members, ks.d_cmt_ids, ks.n_cmt_ids, ks.d_cmt_span_off, ks.d_bits, ks.bits_stride, c->cmt_route_mode, list, ls,
                               irec, n, s);
        mbls_cms_launch_aggregate(ws, ks.d_recs, ks.tsize, list, ls, irec, ks.d_crecs, ks.d_cmt_ids, ks.d_cmt_span_off, c->d_cms_park + tk.ws_off, c->cms_items, st, n, s);
    } else if (ks.committee) {
        // the items' lists in the scratch reserved for the whole plan (reserve_committee: nothing grows under a pass in flight), at the pass's workspace offset
        const uint64_t ls = ks.cmax ? ks.cmax : 1;
        if ((tk.ws_off + n) * ls > c->cmt_words || tk.ws_off + n > c->cmt_items) ARGFAIL(c, "internal: the committee scratch of a pass was not reserved");
        rc = committees_acquire(c, ks.cmt, s); if (rc) return rc;
        uint32_t* const list = c->d_cmt_list + tk.ws_off * ls; uint32_t* const cnt = c->d_cmt_cnt + tk.ws_off; uint32_t* const route = c->d_cmt_cnt + c->cmt_items + tk.ws_off;
        hipLaunchKernelGGL(k_cmt_expand, dim3((unsigned)n), dim3(WG), 0, s, ks.d_crecs, ks.ccount, ks.d_members, ks.d_cmt_idx, ks.d_bits, ks.bits_stride, c->cmt_route_mode,
                           list, ls, cnt, route, n);
        hipLaunchKernelGGL(k_aggregate_cmt_d, dim3(g), dim3(WG), 0, s, ws, ks.d_recs, ks.tsize, (const uint32_t*)list, ls, (const uint32_t*)cnt, (const uint32_t*)route,
                           ks.d_crecs, ks.d_cmt_idx, st, n);
    } else if (key_split) {
        mbls_ws wsub = ws; wsub.w += n;                                  // sub-item t = workspace item n + t (APK slots only; nothing else uses them up there)
        uint32_t* st_sub = c->d_status + tk.ws_off + n;                  // their status words: behind the items' own
        HIPCHK(c, hipMemsetAsync(st_sub, 0, 4 * nsub, s));
        if (ks.indexed)
            hipLaunchKernelGGL(k_aggregate_indexed_d, dim3(nblk(nsub)), dim3(WG), 0, s, wsub, ks.d_recs, ks.tsize, ks.d_idx, (const uint32_t*)nullptr, k / MBLS_KEY_SPLIT,
                               MBLS_MODE_VERIFY, st_sub, nsub);
        else
            hipLaunchKernelGGL(k_aggregate_raw_d, dim3(nblk(nsub)), dim3(WG), 0, s, wsub, ks.d_pks, (const uint32_t*)nullptr, k / MBLS_KEY_SPLIT, MBLS_MODE_VERIFY, st_sub, nsub);
        hipLaunchKernelGGL(k_apk_combine, dim3(g), dim3(WG), 0, s, ws, n, mode, (const uint32_t*)st_sub, st);
    } else if (ks.indexed)
        hipLaunchKernelGGL(k_aggregate_indexed_d, dim3(g), dim3(WG), 0, s, ws, ks.d_recs, ks.tsize, ks.d_idx, d_off, k, mode, st, n);
    else if (staged) {
        hipLaunchKernelGGL(k_pk_decompress, dim3(nblk(n * (uint64_t)k)), dim3(WG), 0, s, ks.d_pks, n * (uint64_t)k, keys_xy, key_flags);
        hipLaunchKernelGGL(k_aggregate_decoded, dim3(g), dim3(WG), 0, s, ws, (const uint32_t*)keys_xy, (const uint8_t*)key_flags, k, mode, st, n);
    } else
        launch_aggregate(ws, ks.d_pks, d_off, k, fmt, mode, st, n, s);
    if (tm) HIPCHK(c, hipEventRecord(c->ev[1], s));
    if (!keys_later) launch_sig();
    if (tm) HIPCHK(c, hipEventRecord(c->ev[2], s));
    if (!keys_later) { rc = launch_msg(); if (rc) return rc; }
    if (tm) HIPCHK(c, hipEventRecord(c->ev[3], s));
    if (fork) {      // join
        if (s_sig != s) { HIPCHK(c, hipEventRecord(tk.ev2, s_sig)); HIPCHK(c, hipStreamWaitEvent(s, tk.ev2, 0)); }
        HIPCHK(c, hipEventRecord(tk.ev3, s_msg)); HIPCHK(c, hipStreamWaitEvent(s, tk.ev3, 0));
    }
    if (on_waves) {
        // small batch: one WAVE per item walks the Miller loop and the final exponentiation with its lanes side by side (mbls_coop.h)
        coop_run(c, pp.pairing == MBLS_PAIRING_WAVE_X2 ? COOP_PAIRING2X2 : COOP_PAIRING2, ws, (uint64_t)0, (uint64_t)1, (uint64_t)0, n, st, d_results, COOP_RES_ITEM, s);
        if (tm) { HIPCHK(c, hipEventRecord(c->ev[4], s)); HIPCHK(c, hipEventRecord(c->ev[5], s)); }
    } else {
        if (split) {
            const int lpp = pp.pairing == MBLS_PAIRING_LANES4 ? 2 : 1;         // a quarter of a round or less: two lanes per pair, products in pairs
            if (lpp == 2) hipLaunchKernelGGL(k_miller_split4, dim3(nblk(4 * n)), dim3(WG), 0, s, ws, n);
            else hipLaunchKernelGGL(k_miller_split, dim3(nblk(2 * n)), dim3(WG), 0, s, ws, n);
            hipLaunchKernelGGL(k_f12_tree_d, dim3(g), dim3(WG), 0, s, ws, 2 * n, n);
            hipLaunchKernelGGL(k_sig_verdict, dim3(g), dim3(WG), 0, s, ws, st, n, n, 1);
        } else {
            hipLaunchKernelGGL(k_miller, dim3(g), dim3(WG), 0, s, ws, n);
            if (fused_sig) hipLaunchKernelGGL(k_sig_verdict, dim3(g), dim3(WG), 0, s, ws, st, n, (uint64_t)0, 0);
        }
        if (tm) HIPCHK(c, hipEventRecord(c->ev[4], s));
        if (split) hipLaunchKernelGGL(k_final2, dim3(nblk(2 * n)), dim3(WG), 0, s, ws, st, d_results, n);      // two lanes per item here too
        else hipLaunchKernelGGL(k_final, dim3(g), dim3(WG), 0, s, ws, st, d_results, n);
        if (tm) HIPCHK(c, hipEventRecord(c->ev[5], s));
    }
    if (d_bitmap) hipLaunchKernelGGL(k_pack, dim3(g), dim3(WG), 0, s, d_results, d_bitmap, n);
    if (tm) {
        HIPCHK(c, hipEventRecord(c->ev[6], s));
        HIPCHK(c, hipEventSynchronize(c->ev[6]));
        for (int i = 0; i < MBLS_N_PHASES; i++) HIPCHK(c, hipEventElapsedTime(&c->phase_ms[i], c->ev[i], c->ev[i + 1]));
    }
    HIPCHK(c, hipGetLastError());
    return tk.ws_sync ? ws_release(c, s) : MBLS_OK;
}
// One growth of the workspace (and of the staging of decompressed keys) for a whole plan, before its first pass is queued: nothing may be reallocated under a pass
// in flight (a pass on the wave engine may take the eight-lane key sum: n + 8 n items -- pass_ws_items, the figure the pass itself acts on; the staging of
// decompressed keys is indexed by ITEM, so it follows the items' extent, not the partial sums'). min_items: what the call needs besides (the hash of a list).
static int reserve_plan(mbls_ctx* c, const mbls_batch_plan& bp, const keysrc& ks, uint32_t k, uint64_t min_items = 0) {
    uint64_t need = min_items, need_items = 0;
    for (uint32_t i = 0; i < bp.n_passes; i++) {
        const uint64_t e = bp.pass[i].workspace_first + pass_ws_items(bp.pass[i], ks, k, bp.pass[i].items); if (e > need) need = e;
        const uint64_t ei = bp.pass[i].workspace_first + bp.pass[i].items; if (ei > need_items) need_items = ei;
    }
    int rc = mbls_ctx_reserve(c, need); if (rc) return rc;
    if (!ks.indexed && ks.fmt == MBLS_PK_COMPRESSED && !ks.d_off && k > 1) return reserve_keys(c, need_items * (uint64_t)k);
    return MBLS_OK;
}
// The batch as the caller sees it: plan_batch decides (see there), this function carries the plan out. Passes of one stage run side by side -- track 0 on the
// caller's stream, track 1 on the context's second set of streams, forked from and joined to the caller's stream --, stages one after the other.
static int verify_pipeline(mbls_ctx* c, const batch& b, hipStream_t s, int part = 0) {
    if (!c || part != 0 || b.n == 0) return verify_pipeline_one(c, b, s, part);
    mbls_batch_plan bp; plan_batch(ctx_limits(c), b.n, c->timing, c->timing, &bp);
    if (bp.mode == MBLS_BATCH_ONE_PASS) return verify_pipeline_one(c, b, s);
    int rc = reserve_plan(c, bp, b.ks, b.k); if (rc) return rc;
    // a pass of the plan: the slice of its items, in the space reserved above
    auto run = [&](const mbls_pass_plan& p, hipStream_t ps, const track* tk) { return verify_pipeline_one(c, slice(b, p.first_item, p.first_item + p.items), ps, 0, tk, true); };
    if (bp.mode == MBLS_BATCH_ROUNDS_THEN_REST) { rc = run(bp.pass[0], s, nullptr); return rc ? rc : run(bp.pass[1], s, nullptr); }
    // two tracks: [rounds in front,] then two passes side by side
    uint32_t i = 0;
    if (bp.n_passes == 3) { rc = run(bp.pass[0], s, nullptr); if (rc) return rc; i = 1; }
    const mbls_pass_plan& pa = bp.pass[i]; const mbls_pass_plan& pb = bp.pass[i + 1];
    const bool side = bp.mode == MBLS_BATCH_ROUND_BESIDE_REST;
    const uint64_t fm = side ? ~0ull : (pa.front == MBLS_FRONT_IN_A_ROW ? 0 : c->fork_max_items);
    rc = ws_acquire(c, s); if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->t1_ev, s)); HIPCHK(c, hipStreamWaitEvent(c->t1_s, c->t1_ev, 0));
    track ta = track0(c); ta.ws_sync = false; ta.fork_max = fm;
    track tb; tb.no_waves = side; tb.fork_max = fm; tb.ws_off = pb.workspace_first; tb.sb = c->t1_b; tb.sc = c->t1_c; tb.sd = c->t1_b; tb.ev2 = c->t1_ev2; tb.ev3 = c->t1_ev3; tb.ws_sync = false;
    if (side) {          // the round first: its kernels fill the chip, the remainder's waves take what they leave between them
        rc = run(pa, s, &ta);
        if (!rc) rc = run(pb, c->t1_s, &tb);
    } else {
        rc = run(pb, c->t1_s, &tb);
        if (!rc) rc = run(pa, s, &ta);
    }
    // join: the caller's stream ends when both tracks have (also on an error path: nothing of the call stays in flight unordered)
    hipError_t e1 = hipEventRecord(c->t1_ev, c->t1_s), e2 = hipStreamWaitEvent(s, c->t1_ev, 0);
    if (rc) return rc;
    HIPCHK(c, e1); HIPCHK(c, e2);
    return ws_release(c, s);
}
extern "C" int mbls_ctx_set_tracks(mbls_ctx* c, uint64_t min_rest_items, uint64_t side_max_items) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu); c->tracks_min_rest = min_rest_items; c->tracks_side_max = side_max_items; return MBLS_OK;
}
// The one way from the nine *_device entries (and from the host stager) into the pipeline. Per-item messages go straight to verify_pipeline. A shared list (the
// call carries n_msgs messages and one index per item: include/mbls.h) is hashed once -- by the same launch_hash, in the form its size asks for (plan_shared) --, its
// points go to the context's table (k_h_export_tab), and the message phase of every pass is the gather (k_h_gather): one-pass plans hash the list inside the pass,
// on its message stream beside the key sum and the signatures; plans of several passes hash it on the caller's stream before the first pass. Everything is reserved
// before anything is queued: the workspace for the larger of the items' plan and the list, the key staging, the table. A resident table (mt) is read at the size
// it has now (the caller holds the context's lock); every stream of the call forks from s behind the table's last append, and nothing is hashed.
static int verify_device(mbls_ctx* c, batch b, const mbls_msgtable* mt, hipStream_t s) {
    msgsrc& ms = b.ms;
    if (b.ks.fmt != MBLS_PK_COMPRESSED && b.ks.fmt != MBLS_PK_UNCOMPRESSED) return MBLS_ERR_ARGUMENT;
    if (b.ks.committee && b.n) {          // the scratch of k_cmt_expand / k_cms_expand for the whole plan (the extent of its passes), before anything is queued
        HIPCHK(c, hipSetDevice(c->device));
        mbls_batch_plan bp; plan_batch(ctx_limits(c), b.n, c->timing, c->timing, &bp);
        uint64_t extent = 0;
        for (uint32_t i = 0; i < bp.n_passes; i++) { const uint64_t e = bp.pass[i].workspace_first + bp.pass[i].items; if (e > extent) extent = e; }
        const int rr = b.ks.span ? reserve_committee_span(c, extent, cms_stride(b.ks.bits_stride, b.ks.cmax)) : reserve_committee(c, extent, b.ks.cmax); if (rr) return rr;
    }
    if (mt) {
        if (mt->c != c) ARGFAIL(c, "message table belongs to another context");
        ms = msgs_of_table(mt, ms.d_idx);
    }
    if (!ms.indexed()) return verify_pipeline(c, b, s);
    if (b.n == 0) return MBLS_OK;
    if (ms.n_msgs > 0xFFFFFFFFull) ARGFAIL(c, "message indices are 32-bit");
    if (!b.d_sigs || !ms.d_idx || !b.d_results || (ms.n_msgs && !ms.d_msgs && ms.msg_len && !ms.d_moff)) ARGFAIL(c, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    if (mt) {            // (verify_pipeline reserves the plan's workspace and key staging before it queues the first pass: there is no list to size here)
        const int ra = msgtable_acquire(c, mt, s); if (ra) return ra;
        return verify_pipeline(c, b, s);
    }
    mbls_shared_msgs_plan sp; plan_shared(ctx_limits(c), b.n, ms.n_msgs, c->timing, c->timing, &sp);
    int rc = reserve_plan(c, sp.batch, b.ks, b.k, sp.list_workspace_items); if (rc) return rc;
    rc = reserve_msgs(c, ms.n_msgs); if (rc) return rc;
    ms.tab = c->d_htab; ms.tstride = c->htab_cap; ms.flags = c->d_hflag;
    if (sp.batch.mode == MBLS_BATCH_ONE_PASS) ms.list = &sp;
    else {
        rc = ws_acquire(c, s); if (rc) return rc;
        rc = shared_hash_list(c, sp, ms.d_msgs, ms.msg_len, ms.d_moff, ms.n_msgs, s); if (rc) return rc;
    }
    return verify_pipeline(c, b, s);
}
extern "C" int mbls_fast_aggregate_verify_batch_device(mbls_ctx* c, const uint8_t* d_sigs, const uint8_t* d_msgs, uint32_t msg_len,
        const uint64_t* d_moff, const uint8_t* d_pks, int fmt, const uint32_t* d_off, uint64_t n, uint32_t k, uint8_t* d_results, uint64_t* d_bitmap,
        uint32_t* d_status, void* stream) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    return verify_device(c, batch{d_sigs, msgs_per_item(d_msgs, msg_len, d_moff), keys_wire(d_pks, fmt, d_off), n, k, MBLS_MODE_FAST_AGGREGATE, d_results, d_bitmap, d_status},
                         nullptr, (hipStream_t)stream);
}
extern "C" int mbls_verify_batch_device(mbls_ctx* c, const uint8_t* d_sigs, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff,
        const uint8_t* d_pks, int fmt, uint64_t n, uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    return verify_device(c, batch{d_sigs, msgs_per_item(d_msgs, msg_len, d_moff), keys_wire(d_pks, fmt, nullptr), n, 1, MBLS_MODE_VERIFY, d_results, d_bitmap, d_status},
                         nullptr, (hipStream_t)stream);
}

// offsets of a ragged key / signature table handed over in host memory: non-decreasing, and the total fits the index type
static bool offsets_ok(const uint32_t* off, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) if (off[i + 1] < off[i]) return false;
    return true;
}
// message ranges: non-decreasing, every message shorter than 2^32 bytes
static bool msg_offsets_ok(const uint64_t* off, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) if (off[i + 1] < off[i] || off[i + 1] - off[i] > 0xFFFFFFFFull) return false;
    return true;
}

// Host buffers in, results out, for every per-item entry. `hm` describes the messages with HOST pointers: the items' own bytes, a list of n_msgs messages plus one
// index per item, or indices into the resident table mt. The tables are checked here (a bad offset table or an index that names nothing refuses the call, nothing
// enqueued), everything is staged through the context's buffers, and the pipeline runs on the context's stream. With per-item messages the keys (or key indices)
// are 99 % of the bytes: they are uploaded on a second stream while the signature and message phases run.
static int verify_host(mbls_ctx* c, const uint8_t* sigs, msgsrc hm, const mbls_msgtable* mt, const uint8_t* pks, int fmt, const mbls_keytable* tab,
                       const uint32_t* idx, const uint32_t* off, uint64_t n, uint32_t k, int mode, uint8_t* results, uint32_t* status,
                       const host_committees* hc = nullptr) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (mt) {            // the table's size and buffers are read under the lock: an append or a clear on another thread comes before or after the whole call
        if (mt->c != c) ARGFAIL(c, "message table belongs to another context");
        hm = msgs_of_table(mt, hm.d_idx);
    }
    if (n == 0) return MBLS_OK;
    const uint8_t* msgs = hm.d_msgs; const uint64_t* moff = hm.d_moff;
    const uint64_t n_own = hm.kind == MBLS_MSGS_LIST ? hm.n_msgs : n;      // the messages whose bytes the call carries (a table's entries: none, msg_len = 0)
    if (hm.kind == MBLS_MSGS_LIST && hm.n_msgs > 0xFFFFFFFFull) ARGFAIL(c, "message indices are 32-bit");
    if (hm.indexed() && (!sigs || !hm.d_idx || !results)) ARGFAIL(c, "null buffer");
    if (moff && !msg_offsets_ok(moff, n_own)) ARGFAIL(c, "msg_offsets must be non-decreasing, messages below 2^32 bytes");
    if (hm.indexed())
        for (uint64_t i = 0; i < n; i++)
            if (mtb_names_nothing(hm.d_idx[i], hm.n_msgs)) ARGFAIL(c, mt ? "msg_idx names no entry of the message table" : "msg_idx names no message of the list");
    const uint64_t msg_first = moff ? moff[0] : 0;                       // the bytes this call uploads: msgs[msg_first .. msg_first + msg_total)
    const size_t msg_total = moff ? (size_t)(moff[n_own] - moff[0]) : (size_t)hm.msg_len * n_own;
    if (!sigs || (!msgs && msg_total) || !results) ARGFAIL(c, "null buffer");
    if (fmt != MBLS_PK_COMPRESSED && fmt != MBLS_PK_UNCOMPRESSED) ARGFAIL(c, "pk_format");
    keysrc ks = keys_wire(nullptr, fmt, nullptr);
    if (tab) { const int rk = keys_of_table(c, tab, nullptr, nullptr, &ks); if (rk) return rk; }
    if (hc && hc->span) {        // keys by committee span: every item's shape is checked here (cms_range_ok, the ids, cms_field_ok), a malformed item refuses the call
        const int rk = keys_of_committee_span(c, hc->t, nullptr, hc->n_cmt_ids, nullptr, nullptr, hc->bits_stride, false, &ks); if (rk) return rk;
        const int ri = committee_span_items_ok(c, *hc, n); if (ri) return ri;
    } else if (hc) {     // keys by committee and bitfield (pks, tab, idx, off null, k = 0): the table read under the lock, an id that names nothing refuses the call
        const int rk = keys_of_committees(c, hc->t, nullptr, nullptr, hc->bits_stride, false, &ks); if (rk) return rk;
        if (!hc->cmt_idx || !hc->bits) ARGFAIL(c, "null buffer");
        for (uint64_t i = 0; i < n; i++) if ((uint64_t)hc->cmt_idx[i] >= hc->t->count) ARGFAIL(c, "cmt_idx names no committee of the table");
    }
    if (off && !offsets_ok(off, n)) ARGFAIL(c, "offsets must be non-decreasing");
    HIPCHK(c, hipSetDevice(c->device));
    // like the messages, a key offset table may start anywhere (a shard of a larger batch): only keys [off[0], off[n]) are uploaded
    const uint64_t key_first = off ? off[0] : 0;
    const uint64_t total_keys = off ? (uint64_t)(off[n] - off[0]) : (uint64_t)k * n;
    const bool indexed = tab != nullptr;
    if (total_keys && !(indexed ? (const void*)idx : (const void*)pks)) ARGFAIL(c, "null key buffer");
    const size_t unit = indexed ? 4 : (fmt == MBLS_PK_COMPRESSED ? 48 : 96);
    const void* h_keys = total_keys ? (indexed ? (const void*)(idx + key_first) : (const void*)(pks + unit * key_first)) : nullptr;
    sbuf ds(c, 0), dm(c, 1), dp(c, 2), doff(c, 3), dr(c, 4), dst(c, 5), dmo(c, 6), dmi(c, 7), dso(c, 8);
    batch b{nullptr, hm, ks, n, k, mode, nullptr, nullptr, nullptr};       // the same batch with DEVICE pointers
    HIPCHK(c, ds.up(sigs, 96 * n)); b.d_sigs = ds.as<uint8_t>();
    if (hm.kind != MBLS_MSGS_TABLE) { HIPCHK(c, dm.up(msgs ? msgs + msg_first : nullptr, msg_total)); b.ms.d_msgs = dm.as<uint8_t>(); }
    if (hm.indexed()) { HIPCHK(c, dmi.up(hm.d_idx, 4 * n)); b.ms.d_idx = dmi.as<uint32_t>(); }
    if (off) { HIPCHK(c, doff.up(off, 4 * (n + 1))); b.ks.d_off = doff.as<uint32_t>(); }
    if (moff) {                                                          // the table as given; the uploaded bytes start at msgs[moff[0]]
        HIPCHK(c, dmo.up(moff, 8 * (n_own + 1))); b.ms.d_moff = dmo.as<uint64_t>(); b.ms.d_msgs -= msg_first;
    }
    HIPCHK(c, dr.alloc(n)); HIPCHK(c, dst.alloc(4 * n)); b.d_results = dr.as<uint8_t>(); b.d_status = dst.as<uint32_t>();
    auto keys_are_there = [&]() { if (indexed) b.ks.d_idx = dp.as<uint32_t>() - key_first; else b.ks.d_pks = dp.as<uint8_t>() - unit * key_first; };     // the table's offsets are absolute
    const bool late_keys = !hm.indexed() && !hc; // (the indexed kinds and the committee form upload their keys up front: the late upload has not been measured for them)
    if (hc && hc->span) {       // the ids and the bitfields take the two key slots, the span offsets one of their own
        HIPCHK(c, dp.up(hc->cmt_ids, 4 * hc->n_cmt_ids)); HIPCHK(c, doff.up(hc->bits, (size_t)hc->bits_stride * n)); HIPCHK(c, dso.up(hc->cmt_off, 4 * (n + 1)));
        b.ks.d_cmt_ids = dp.as<uint32_t>(); b.ks.d_bits = doff.as<uint8_t>(); b.ks.d_cmt_span_off = dso.as<uint32_t>();
    } else if (hc) {     // the ids and the bitfields take the two key slots
        HIPCHK(c, dp.up(hc->cmt_idx, 4 * n)); HIPCHK(c, doff.up(hc->bits, (size_t)hc->bits_stride * n));
        b.ks.d_cmt_idx = dp.as<uint32_t>(); b.ks.d_bits = doff.as<uint8_t>();
    } else if (late_keys) HIPCHK(c, dp.alloc(unit * total_keys)); else { HIPCHK(c, dp.up(h_keys, unit * total_keys)); keys_are_there(); }
    const bool tm = c->timing; c->timing = false;        // the phase timers assume the plain order, on the device entries
    int rc;
    if (!late_keys) rc = verify_device(c, b, mt, c->hs_a);
    else {
        const uint64_t R = c->round_items;
        const uint64_t n_head = (R && n > R && n % R) ? n - n % R : n;   // the rounds first (parts 1 and 2 below); the remainder as a full pass once the keys are there
        rc = verify_pipeline(c, slice(b, 0, n_head), c->hs_a, 1);
        if (!rc) {
            hipError_t e1 = hipSuccess;      // issued after the first two phases were queued: a copy from pageable memory may block the host
            if (total_keys) e1 = hipMemcpyAsync(dp.p, h_keys, unit * total_keys, hipMemcpyHostToDevice, c->hs_b);
            if (e1 == hipSuccess) e1 = hipEventRecord(c->hs_ev, c->hs_b);
            if (e1 == hipSuccess) e1 = hipStreamWaitEvent(c->hs_a, c->hs_ev, 0);
            if (e1 != hipSuccess) { snprintf(c->err, sizeof(c->err), "key upload failed: %s", hipGetErrorString(e1)); rc = MBLS_ERR_DEVICE; }
        }
        if (!rc) {
            keys_are_there();
            rc = verify_pipeline(c, slice(b, 0, n_head), c->hs_a, 2);
            if (!rc && n_head < n) rc = verify_pipeline_one(c, slice(b, n_head, n), c->hs_a);
        }
    }
    c->timing = tm;
    if (rc) {         // passes may be running on the context's streams and its second track: nothing of this call is left in flight when it returns an error
        (void)hipStreamSynchronize(c->hs_a); (void)hipStreamSynchronize(c->hs_b); (void)hipStreamSynchronize(c->hs_c); (void)hipStreamSynchronize(c->hs_d);
        (void)hipStreamSynchronize(c->t1_s);
        c->ws_pending = false;
        return rc;
    }
    HIPCHK(c, hipStreamSynchronize(c->hs_a));
    c->ws_pending = false;
    HIPCHK(c, dr.down(results, n));
    if (status) HIPCHK(c, dst.down(status, 4 * n));
    return MBLS_OK;
}
extern "C" int mbls_fast_aggregate_verify_batch(mbls_ctx* c, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len, const uint64_t* moff,
        const uint8_t* pks, int fmt, const uint32_t* off, uint64_t n, uint32_t k, uint8_t* results, uint32_t* status) {
    return verify_host(c, sigs, msgs_per_item(msgs, msg_len, moff), nullptr, pks, fmt, nullptr, nullptr, off, n, k, MBLS_MODE_FAST_AGGREGATE, results, status);
}
extern "C" int mbls_verify_batch(mbls_ctx* c, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len, const uint64_t* moff, const uint8_t* pks, int fmt,
        uint64_t n, uint8_t* results, uint32_t* status) {
    return verify_host(c, sigs, msgs_per_item(msgs, msg_len, moff), nullptr, pks, fmt, nullptr, nullptr, nullptr, n, 1, MBLS_MODE_VERIFY, results, status);
}

// ---- resident key table
extern "C" int mbls_keytable_create(mbls_ctx* c, uint64_t capacity_hint, mbls_keytable** out) {
    if (!c || !out) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    mbls_keytable* t = new (std::nothrow) mbls_keytable();
    if (!t) return MBLS_ERR_DEVICE;
    t->c = c; t->cap = capacity_hint ? capacity_hint : 1024;
    hipError_t e = hipMalloc(&t->d_recs, t->cap * MBLS_KEYREC_DWORDS * 4);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t->ev, hipEventDisableTiming);
    if (e != hipSuccess) { if (t->d_recs) (void)hipFree(t->d_recs); delete t; HIPCHK(c, e); }
    try { c->tables.push_back(t); } catch (...) { (void)hipFree(t->d_recs); (void)hipEventDestroy(t->ev); delete t; return MBLS_ERR_DEVICE; }
    *out = t; return MBLS_OK;
}
// Either order of destruction is fine: a table whose context went first is an empty shell (mbls_ctx_destroy released its records).
extern "C" void mbls_keytable_destroy(mbls_keytable* t) {
    if (!t) return;
    if (t->c) {
        mbls_ctx* c = t->c;
        mbls_lock lk(c->mu); (void)hipSetDevice(c->device); (void)hipDeviceSynchronize();
        if (t->d_recs) (void)hipFree(t->d_recs);
        if (t->ev) (void)hipEventDestroy(t->ev);
        for (size_t i = 0; i < c->tables.size(); i++) if (c->tables[i] == t) { c->tables.erase(c->tables.begin() + i); break; }
        for (mbls_committees* ct : c->committees) if (ct->kt == t) ct->kt = nullptr;      // committee tables still bound to it: unbound, they refuse appends and verifications
    }
    delete t;
}
// undo of an append (mbls_multi_keytable_append: a replica failed): later appends overwrite the dropped records
static void keytable_truncate(mbls_keytable* t, uint64_t size) {
    if (!t || !t->c) return;
    mbls_lock lk(t->c->mu);
    if (size < t->size) t->size = size;
}
extern "C" uint64_t mbls_keytable_size(const mbls_keytable* t) { if (!t || !t->c) return 0; mbls_lock lk(t->c->mu); return t->size; }
static int keytable_grow(mbls_keytable* t, uint64_t need, hipStream_t s) {
    mbls_ctx* c = t->c;
    if (need <= t->cap) return MBLS_OK;
    uint64_t ncap = t->cap * 2 > need ? t->cap * 2 : need;
    uint32_t* nr = nullptr;
    HIPCHK(c, hipMalloc(&nr, ncap * MBLS_KEYREC_DWORDS * 4));
    // appends in flight on other streams must have written the old records before they are copied, and verifications in flight may
    // still read them when they are freed: the device is drained on both sides of the copy (growth is rare; reserve with capacity_hint)
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess && t->size) e = hipMemcpyAsync(nr, t->d_recs, t->size * MBLS_KEYREC_DWORDS * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) t->pending = false;
    if (e != hipSuccess) { (void)hipFree(nr); HIPCHK(c, e); }
    (void)hipFree(t->d_recs); t->d_recs = nr; t->cap = ncap;
    return MBLS_OK;
}
extern "C" int mbls_keytable_append_device(mbls_keytable* t, const uint8_t* d_pks, int fmt, int validate, uint64_t n, uint64_t* first_index,
                                           uint8_t* d_errs, void* stream) {
    if (!t || !t->c) return MBLS_ERR_ARGUMENT;
    mbls_ctx* c = t->c;
    mbls_lock lk(c->mu);
    if ((fmt != MBLS_PK_COMPRESSED && fmt != MBLS_PK_UNCOMPRESSED) || (n && (!d_pks || !d_errs))) ARGFAIL(c, "keytable_append");
    if (t->size + n > 0xFFFFFFFFull) ARGFAIL(c, "key table indices are 32-bit");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    int rc = keytable_grow(t, t->size + n, s); if (rc) return rc;
    if (n) {
        // an earlier append on another stream may still be writing its own records: nothing to order (disjoint), but the event below
        // replaces the earlier one, so this stream inherits the earlier append's completion first
        if (t->pending && t->ev_stream != s) HIPCHK(c, hipStreamWaitEvent(s, t->ev, 0));
        hipLaunchKernelGGL(k_keytable_append, dim3(nblk(n)), dim3(WG), 0, s, d_pks, fmt, validate, n, t->d_recs + t->size * MBLS_KEYREC_DWORDS, d_errs);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(t->ev, s)); t->ev_stream = s; t->pending = true;     // readers on other streams wait for this (table_acquire)
    }
    if (first_index) *first_index = t->size;      // published only once everything of the append is in the stream
    t->size += n; return MBLS_OK;
}
static int map_dec_err_g1(int e) { return e == MBLS_DEC_OK ? MBLS_OK : (e == MBLS_DEC_SIZE ? MBLS_ERR_INVALID_G1_SIZE : MBLS_ERR_INVALID_POINT); }
static int map_dec_err_g2(int e) { return e == MBLS_DEC_OK ? MBLS_OK : (e == MBLS_DEC_SIZE ? MBLS_ERR_INVALID_G2_SIZE : MBLS_ERR_INVALID_POINT); }
extern "C" int mbls_keytable_append(mbls_keytable* t, const uint8_t* pks, int fmt, int validate, uint64_t n, uint64_t* first_index, uint8_t* errs) {
    if (!t || !t->c) return MBLS_ERR_ARGUMENT;
    mbls_ctx* c = t->c;
    mbls_lock lk(c->mu);
    if ((fmt != MBLS_PK_COMPRESSED && fmt != MBLS_PK_UNCOMPRESSED) || (n && (!pks || !errs))) ARGFAIL(c, "keytable_append");
    HIPCHK(c, hipSetDevice(c->device));
    sbuf di(c, 0), de(c, 1);
    HIPCHK(c, di.up(pks, (fmt ? 96 : 48) * n)); HIPCHK(c, de.alloc(n));
    int rc = mbls_keytable_append_device(t, di.as<uint8_t>(), fmt, validate, n, first_index, de.as<uint8_t>(), c->hs_a); if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->hs_a)); HIPCHK(c, de.down(errs, n));
    if (t->ev_stream == c->hs_a) t->pending = false;
    for (uint64_t i = 0; i < n; i++) errs[i] = (uint8_t)map_dec_err_g1(errs[i]);
    return MBLS_OK;
}
extern "C" int mbls_keytable_get(mbls_keytable* t, uint64_t first, uint64_t n, uint8_t* pks96, uint8_t* errs) {
    if (!t || !t->c) return MBLS_ERR_ARGUMENT;
    mbls_ctx* c = t->c;
    mbls_lock lk(c->mu);
    if (first + n > t->size || (n && (!pks96 || !errs))) ARGFAIL(c, "keytable_get range");
    if (!n) return MBLS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    sbuf dout(c, 0), de(c, 1); HIPCHK(c, dout.alloc(96 * n)); HIPCHK(c, de.alloc(n));
    { int rc = table_acquire(c, t, c->hs_a); if (rc) return rc; }
    hipLaunchKernelGGL(k_keytable_export, dim3(nblk(n)), dim3(WG), 0, c->hs_a, (const uint32_t*)t->d_recs, first, n, dout.as<uint8_t>(), de.as<uint8_t>());
    HIPCHK(c, hipStreamSynchronize(c->hs_a)); HIPCHK(c, dout.down(pks96, 96 * n)); HIPCHK(c, de.down(errs, n));
    for (uint64_t i = 0; i < n; i++) errs[i] = (uint8_t)map_dec_err_g1(errs[i]);
    return MBLS_OK;
}
extern "C" int mbls_fast_aggregate_verify_batch_indexed_device(mbls_ctx* c, const mbls_keytable* t, const uint8_t* d_sigs, const uint8_t* d_msgs,
        uint32_t msg_len, const uint64_t* d_moff, const uint32_t* d_idx, const uint32_t* d_off, uint64_t n, uint32_t k, uint8_t* d_results, uint64_t* d_bitmap,
        uint32_t* d_status, void* stream) {
    if (!c || !t) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    keysrc ks; const int rk = keys_of_table(c, t, d_idx, d_off, &ks); if (rk) return rk;
    return verify_device(c, batch{d_sigs, msgs_per_item(d_msgs, msg_len, d_moff), ks, n, k, MBLS_MODE_FAST_AGGREGATE, d_results, d_bitmap, d_status}, nullptr, (hipStream_t)stream);
}
extern "C" int mbls_fast_aggregate_verify_batch_indexed(mbls_ctx* c, const mbls_keytable* t, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len,
        const uint64_t* moff, const uint32_t* idx, const uint32_t* off, uint64_t n, uint32_t k, uint8_t* results, uint32_t* status) {
    if (!c || !t) return MBLS_ERR_ARGUMENT;
    return verify_host(c, sigs, msgs_per_item(msgs, msg_len, moff), nullptr, nullptr, MBLS_PK_UNCOMPRESSED, t, idx, off, n, k, MBLS_MODE_FAST_AGGREGATE, results, status);
}

// ---- shared message lists: the call carries n_msgs messages and one index per item (include/mbls.h); how they run: verify_device
extern "C" int mbls_fast_aggregate_verify_batch_shared_msgs_device(mbls_ctx* c, const uint8_t* d_sigs, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff,
        uint64_t n_msgs, const uint32_t* d_msg_idx, const uint8_t* d_pks, int fmt, const uint32_t* d_off, uint64_t n, uint32_t k, uint8_t* d_results, uint64_t* d_bitmap,
        uint32_t* d_status, void* stream) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    return verify_device(c, batch{d_sigs, msgs_list(d_msgs, msg_len, d_moff, n_msgs, d_msg_idx), keys_wire(d_pks, fmt, d_off), n, k, MBLS_MODE_FAST_AGGREGATE, d_results, d_bitmap,
                         d_status}, nullptr, (hipStream_t)stream);
}
extern "C" int mbls_verify_batch_shared_msgs_device(mbls_ctx* c, const uint8_t* d_sigs, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff, uint64_t n_msgs,
        const uint32_t* d_msg_idx, const uint8_t* d_pks, int fmt, uint64_t n, uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    return verify_device(c, batch{d_sigs, msgs_list(d_msgs, msg_len, d_moff, n_msgs, d_msg_idx), keys_wire(d_pks, fmt, nullptr), n, 1, MBLS_MODE_VERIFY, d_results, d_bitmap, d_status},
                         nullptr, (hipStream_t)stream);
}
extern "C" int mbls_fast_aggregate_verify_batch_indexed_shared_msgs_device(mbls_ctx* c, const mbls_keytable* t, const uint8_t* d_sigs, const uint8_t* d_msgs, uint32_t msg_len,
        const uint64_t* d_moff, uint64_t n_msgs, const uint32_t* d_msg_idx, const uint32_t* d_idx, const uint32_t* d_off, uint64_t n, uint32_t k, uint8_t* d_results,
        uint64_t* d_bitmap, uint32_t* d_status, void* stream) {
    if (!c || !t) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    keysrc ks; const int rk = keys_of_table(c, t, d_idx, d_off, &ks); if (rk) return rk;
    return verify_device(c, batch{d_sigs, msgs_list(d_msgs, msg_len, d_moff, n_msgs, d_msg_idx), ks, n, k, MBLS_MODE_FAST_AGGREGATE, d_results, d_bitmap, d_status}, nullptr,
                         (hipStream_t)stream);
}
extern "C" int mbls_fast_aggregate_verify_batch_shared_msgs(mbls_ctx* c, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len, const uint64_t* moff, uint64_t n_msgs,
        const uint32_t* msg_idx, const uint8_t* pks, int fmt, const uint32_t* off, uint64_t n, uint32_t k, uint8_t* results, uint32_t* status) {
    return verify_host(c, sigs, msgs_list(msgs, msg_len, moff, n_msgs, msg_idx), nullptr, pks, fmt, nullptr, nullptr, off, n, k, MBLS_MODE_FAST_AGGREGATE, results, status);
}
extern "C" int mbls_verify_batch_shared_msgs(mbls_ctx* c, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len, const uint64_t* moff, uint64_t n_msgs,
        const uint32_t* msg_idx, const uint8_t* pks, int fmt, uint64_t n, uint8_t* results, uint32_t* status) {
    return verify_host(c, sigs, msgs_list(msgs, msg_len, moff, n_msgs, msg_idx), nullptr, pks, fmt, nullptr, nullptr, nullptr, n, 1, MBLS_MODE_VERIFY, results, status);
}
extern "C" int mbls_fast_aggregate_verify_batch_indexed_shared_msgs(mbls_ctx* c, const mbls_keytable* t, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len,
        const uint64_t* moff, uint64_t n_msgs, const uint32_t* msg_idx, const uint32_t* idx, const uint32_t* off, uint64_t n, uint32_t k, uint8_t* results, uint32_t* status) {
    if (!c || !t) return MBLS_ERR_ARGUMENT;
    return verify_host(c, sigs, msgs_list(msgs, msg_len, moff, n_msgs, msg_idx), nullptr, nullptr, MBLS_PK_UNCOMPRESSED, t, idx, off, n, k, MBLS_MODE_FAST_AGGREGATE, results,
                       status);
}

// ---- resident message table (include/mbls.h, mbls_msgtable_*): the message side's key table. An append hashes its messages with launch_hash in the form THEIR count
// asks for (plan_shared's list rule), in the context's workspace, and exports the points behind the entries the table holds (k_h_export_tab at first_index + 1); the
// verification entries take mbls_plan_batch's plan with every pass's message phase the gather from the table (k_h_gather), and hash nothing. Ordering is the key
// table's: an append records an event, readers and later appends on other streams wait for it on the device. Index arithmetic and growth: mbls_mtb.h.
static void msgtable_free_buffers(mbls_msgtable* t) {
    if (t->d_tab) (void)hipFree(t->d_tab);
    if (t->d_flag) (void)hipFree(t->d_flag);
    if (t->d_st) (void)hipFree(t->d_st);
    t->d_tab = t->d_flag = t->d_st = nullptr;
}
static hipError_t msgtable_alloc(uint64_t cap, uint32_t** tab, uint32_t** flag, uint32_t** st) {
    const uint64_t stride = mtb_stride(cap);
    *tab = *flag = *st = nullptr;
    hipError_t e = hipMalloc(tab, (size_t)MBLS_H_DWORDS * stride * 4);
    if (e == hipSuccess) e = hipMalloc(flag, stride * 4);
    if (e == hipSuccess) e = hipMalloc(st, stride * 4);
    if (e != hipSuccess) { if (*tab) (void)hipFree(*tab); if (*flag) (void)hipFree(*flag); if (*st) (void)hipFree(*st); *tab = *flag = *st = nullptr; }
    return e;
}
extern "C" int mbls_msgtable_create(mbls_ctx* c, uint64_t capacity_hint, mbls_msgtable** out) {
    if (!c || !out) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (capacity_hint > 0xFFFFFFFFull) ARGFAIL(c, "message table indices are 32-bit");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = mbls_ctx_reserve(c, 1); if (rc) return rc;
    mbls_msgtable* t = new (std::nothrow) mbls_msgtable();
    if (!t) return MBLS_ERR_DEVICE;
    t->c = c; t->cap = capacity_hint ? capacity_hint : MBLS_MTB_DEFAULT_CAPACITY;
    hipError_t e = msgtable_alloc(t->cap, &t->d_tab, &t->d_flag, &t->d_st);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t->ev, hipEventDisableTiming);
    // the private entry: H of the empty message, hashed here once (growth carries it along, clear keeps it)
    if (e == hipSuccess) {
        hipStream_t s = c->hs_a;
        mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
        if (c->ws_pending && c->ws_stream != s) e = hipStreamWaitEvent(s, c->ws_ev, 0);
        if (e == hipSuccess) e = hipMemsetAsync(t->d_st, 0, 4, s);
        if (e == hipSuccess) {
            launch_hash(c, ws, (const uint8_t*)t->d_tab, 0u, (const uint64_t*)nullptr, t->d_st, (uint64_t)1, s);
            hipLaunchKernelGGL(k_h_export_tab, dim3(1), dim3(MBLS_HB), 0, s, ws, t->d_tab, mtb_stride(t->cap), t->d_flag, (const uint32_t*)t->d_st, (uint64_t)0, (uint64_t)1);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e == hipSuccess) c->ws_pending = false;
    }
    if (e != hipSuccess) { msgtable_free_buffers(t); if (t->ev) (void)hipEventDestroy(t->ev); delete t; HIPCHK(c, e); }
    try { c->msgtables.push_back(t); } catch (...) { msgtable_free_buffers(t); (void)hipEventDestroy(t->ev); delete t; return MBLS_ERR_DEVICE; }
    *out = t; return MBLS_OK;
}
extern "C" void mbls_msgtable_destroy(mbls_msgtable* t) {
    if (!t) return;
    if (t->c) {
        mbls_ctx* c = t->c;
        mbls_lock lk(c->mu); (void)hipSetDevice(c->device); (void)hipDeviceSynchronize();
        msgtable_free_buffers(t);
        if (t->ev) (void)hipEventDestroy(t->ev);
        for (size_t i = 0; i < c->msgtables.size(); i++) if (c->msgtables[i] == t) { c->msgtables.erase(c->msgtables.begin() + i); break; }
    }
    delete t;
}
extern "C" uint64_t mbls_msgtable_size(const mbls_msgtable* t) { if (!t || !t->c) return 0; mbls_lock lk(t->c->mu); return t->size; }
// the count of calls that streams bound to the table have taken and not completed (mbls_stream.hip; hidden: not exported from the library)
extern "C" __attribute__((visibility("hidden"))) void mblsi_msgtable_stream_calls(mbls_msgtable* t, long long delta) { if (t) t->stream_calls.fetch_add(delta); }
// growth keeps every index and entry: new buffers of the new stride, every entry moved by k_mtb_relayout; the device is drained on both sides, like keytable_grow
static int msgtable_grow(mbls_msgtable* t, uint64_t need, hipStream_t s) {
    mbls_ctx* c = t->c;
    const uint64_t ncap = mtb_grown(t->cap, need);
    if (ncap == t->cap) return MBLS_OK;
    uint32_t *nt, *nf, *ns;
    HIPCHK(c, msgtable_alloc(ncap, &nt, &nf, &ns));
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) {
        const uint64_t entries = t->size + 1;
        hipLaunchKernelGGL(k_mtb_relayout, dim3((unsigned)((entries + MBLS_HB - 1) / MBLS_HB)), dim3(MBLS_HB), 0, s, (const uint32_t*)t->d_tab, mtb_stride(t->cap),
                           (const uint32_t*)t->d_flag, nt, mtb_stride(ncap), nf, entries);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { (void)hipFree(nt); (void)hipFree(nf); (void)hipFree(ns); HIPCHK(c, e); }
    t->pending = false;
    msgtable_free_buffers(t);
    t->d_tab = nt; t->d_flag = nf; t->d_st = ns; t->cap = ncap;
    return MBLS_OK;
}
extern "C" int mbls_msgtable_append_device(mbls_msgtable* t, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff, uint64_t n, uint64_t* first_index, void* stream) {
    if (!t || !t->c) return MBLS_ERR_ARGUMENT;
    mbls_ctx* c = t->c;
    mbls_lock lk(c->mu);
    if (n && !d_msgs && msg_len && !d_moff) ARGFAIL(c, "null buffer");
    if (t->size + n > 0xFFFFFFFFull) ARGFAIL(c, "message table indices are 32-bit");
    if (!n) { if (first_index) *first_index = t->size; return MBLS_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    // the form of the hash is the list rule of plan_shared for a list of n messages: pieces of at most one round; wave engine, lane pairs or k_hash
    mbls_shared_msgs_plan sp; plan_shared(ctx_limits(c), 1, n, true, false, &sp);
    int rc = mbls_ctx_reserve(c, sp.list_workspace_items); if (rc) return rc;
    rc = msgtable_grow(t, t->size + n, s); if (rc) return rc;
    rc = ws_acquire(c, s); if (rc) return rc;
    rc = msgtable_acquire(c, t, s); if (rc) return rc;      // the event below replaces the earlier append's: this stream inherits its completion first
    const htab_dst dst = {t->d_tab, mtb_stride(t->cap), t->d_flag, t->d_st, mtb_append_entry(t->size, 0)};
    rc = shared_hash_list(c, sp, d_msgs, msg_len, d_moff, n, s, &dst); if (rc) return rc;
    rc = ws_release(c, s); if (rc) return rc;
    HIPCHK(c, hipEventRecord(t->ev, s)); t->ev_stream = s; t->pending = true;
    if (first_index) *first_index = t->size;
    t->size += n; return MBLS_OK;
}
extern "C" int mbls_msgtable_append(mbls_msgtable* t, const uint8_t* msgs, uint32_t msg_len, const uint64_t* moff, uint64_t n, uint64_t* first_index) {
    if (!t || !t->c) return MBLS_ERR_ARGUMENT;
    mbls_ctx* c = t->c;
    mbls_lock lk(c->mu);
    if (!n) { if (first_index) *first_index = t->size; return MBLS_OK; }
    if (moff && !msg_offsets_ok(moff, n)) ARGFAIL(c, "msg_offsets must be non-decreasing, messages below 2^32 bytes");
    const uint64_t msg_first = moff ? moff[0] : 0;
    const size_t msg_total = moff ? (size_t)(moff[n] - moff[0]) : (size_t)msg_len * n;
    if (!msgs && msg_total) ARGFAIL(c, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    sbuf dm(c, 1), dmo(c, 6);
    HIPCHK(c, dm.up(msgs ? msgs + msg_first : nullptr, msg_total));
    const uint64_t* d_moff = nullptr; const uint8_t* d_msgs = dm.as<uint8_t>();
    if (moff) { HIPCHK(c, dmo.up(moff, 8 * (n + 1))); d_moff = dmo.as<uint64_t>(); d_msgs -= msg_first; }
    const int rc = mbls_msgtable_append_device(t, d_msgs, msg_len, d_moff, n, first_index, c->hs_a);
    const hipError_t e = hipStreamSynchronize(c->hs_a);       // the staged bytes are read until the hash has run
    if (rc) return rc;
    HIPCHK(c, e);
    c->ws_pending = false;
    if (t->ev_stream == c->hs_a) t->pending = false;
    return MBLS_OK;
}
extern "C" int mbls_msgtable_get(mbls_msgtable* t, uint64_t first, uint64_t n, uint8_t* out96, uint8_t* errs) {
    if (!t || !t->c) return MBLS_ERR_ARGUMENT;
    mbls_ctx* c = t->c;
    mbls_lock lk(c->mu);
    if (first > t->size || n > t->size - first || (n && (!out96 || !errs))) ARGFAIL(c, "msgtable_get range");
    if (!n) return MBLS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    sbuf dout(c, 0), de(c, 1); HIPCHK(c, dout.alloc(96 * n)); HIPCHK(c, de.alloc(n));
    int rc = mbls_ctx_reserve(c, n); if (rc) return rc;
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    hipStream_t s = c->hs_a;
    rc = ws_acquire(c, s); if (rc) return rc;
    rc = msgtable_acquire(c, t, s); if (rc) return rc;
    hipLaunchKernelGGL(k_mtb_get, dim3((unsigned)((n + MBLS_HB - 1) / MBLS_HB)), dim3(MBLS_HB), 0, s, ws, (const uint32_t*)t->d_tab, mtb_stride(t->cap), (const uint32_t*)t->d_flag,
                       first, t->size, de.as<uint8_t>(), n);
    hipLaunchKernelGGL(k_h_export, dim3(nblk(n)), dim3(WG), 0, s, ws, n, dout.as<uint8_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s)); c->ws_pending = false;
    HIPCHK(c, dout.down(out96, 96 * n)); HIPCHK(c, de.down(errs, n));
    return MBLS_OK;
}
extern "C" int mbls_msgtable_clear(mbls_msgtable* t) {
    if (!t || !t->c) return MBLS_ERR_ARGUMENT;
    mbls_ctx* c = t->c;
    mbls_lock lk(c->mu);
    if (t->stream_calls.load() > 0) ARGFAIL(c, "msgtable_clear: a stream bound to the table has calls that have not completed");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());           // everything enqueued that reads (or still writes) the table
    t->size = 0; t->pending = false; c->ws_pending = false;
    return MBLS_OK;
}
// the verification entries over a table: mbls_plan_batch's plan, every pass's message phase the gather; the table is read at the size it has now (verify_device).
// The host forms refuse an index that names no entry before anything is enqueued (verify_host).
extern "C" int mbls_fast_aggregate_verify_batch_msgtable_device(mbls_ctx* c, const uint8_t* d_sigs, const mbls_msgtable* mt, const uint32_t* d_msg_idx, const uint8_t* d_pks,
        int fmt, const uint32_t* d_off, uint64_t n, uint32_t k, uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream) {
    if (!c || !mt) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    return verify_device(c, batch{d_sigs, msgs_in_table(d_msg_idx), keys_wire(d_pks, fmt, d_off), n, k, MBLS_MODE_FAST_AGGREGATE, d_results, d_bitmap, d_status}, mt,
                         (hipStream_t)stream);
}
extern "C" int mbls_verify_batch_msgtable_device(mbls_ctx* c, const uint8_t* d_sigs, const mbls_msgtable* mt, const uint32_t* d_msg_idx, const uint8_t* d_pks, int fmt,
        uint64_t n, uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream) {
    if (!c || !mt) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    return verify_device(c, batch{d_sigs, msgs_in_table(d_msg_idx), keys_wire(d_pks, fmt, nullptr), n, 1, MBLS_MODE_VERIFY, d_results, d_bitmap, d_status}, mt, (hipStream_t)stream);
}
extern "C" int mbls_fast_aggregate_verify_batch_indexed_msgtable_device(mbls_ctx* c, const mbls_keytable* t, const uint8_t* d_sigs, const mbls_msgtable* mt,
        const uint32_t* d_msg_idx, const uint32_t* d_idx, const uint32_t* d_off, uint64_t n, uint32_t k, uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream) {
    if (!c || !t || !mt) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    keysrc ks; const int rk = keys_of_table(c, t, d_idx, d_off, &ks); if (rk) return rk;
    return verify_device(c, batch{d_sigs, msgs_in_table(d_msg_idx), ks, n, k, MBLS_MODE_FAST_AGGREGATE, d_results, d_bitmap, d_status}, mt, (hipStream_t)stream);
}
extern "C" int mbls_fast_aggregate_verify_batch_msgtable(mbls_ctx* c, const uint8_t* sigs, const mbls_msgtable* mt, const uint32_t* msg_idx, const uint8_t* pks, int fmt,
        const uint32_t* off, uint64_t n, uint32_t k, uint8_t* results, uint32_t* status) {
    if (!c || !mt) return MBLS_ERR_ARGUMENT;
    return verify_host(c, sigs, msgs_in_table(msg_idx), mt, pks, fmt, nullptr, nullptr, off, n, k, MBLS_MODE_FAST_AGGREGATE, results, status);
}
extern "C" int mbls_verify_batch_msgtable(mbls_ctx* c, const uint8_t* sigs, const mbls_msgtable* mt, const uint32_t* msg_idx, const uint8_t* pks, int fmt, uint64_t n,
        uint8_t* results, uint32_t* status) {
    if (!c || !mt) return MBLS_ERR_ARGUMENT;
    return verify_host(c, sigs, msgs_in_table(msg_idx), mt, pks, fmt, nullptr, nullptr, nullptr, n, 1, MBLS_MODE_VERIFY, results, status);
}
extern "C" int mbls_fast_aggregate_verify_batch_indexed_msgtable(mbls_ctx* c, const mbls_keytable* t, const uint8_t* sigs, const mbls_msgtable* mt, const uint32_t* msg_idx,
        const uint32_t* idx, const uint32_t* off, uint64_t n, uint32_t k, uint8_t* results, uint32_t* status) {
    if (!c || !t || !mt) return MBLS_ERR_ARGUMENT;
    return verify_host(c, sigs, msgs_in_table(msg_idx), mt, nullptr, MBLS_PK_UNCOMPRESSED, t, idx, off, n, k, MBLS_MODE_FAST_AGGREGATE, results, status);
}

// ---- committee table (include/mbls.h, mbls_committees_*; arithmetic: mbls_cmt.h, device bodies: mbls_cmt_lanes.h). The member lists of every committee lie back to
// back in d_members, one record per committee holds where its list starts, its size, the eligible flag and the full key sum. An append uploads the lists, sums them
// with k_aggregate_indexed_d in the context's workspace and lets k_cmt_build write the records; ordering is the key table's (event, readers wait on the device).
extern "C" int mbls_committees_create(mbls_ctx* c, mbls_keytable* kt, uint64_t capacity_hint, mbls_committees** out) {
    if (!c || !kt || !out) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (kt->c != c) ARGFAIL(c, "key table belongs to another context");
    if (capacity_hint > 0xFFFFFFFFull) ARGFAIL(c, "committee ids are 32-bit");
    HIPCHK(c, hipSetDevice(c->device));
    mbls_committees* t = new (std::nothrow) mbls_committees();
    if (!t) return MBLS_ERR_DEVICE;
    t->c = c; t->kt = kt; t->cap = capacity_hint ? capacity_hint : 64; t->members_cap = t->cap * 128;
    hipError_t e = hipMalloc(&t->d_recs, t->cap * MBLS_CMT_REC_DWORDS * 4);
    if (e == hipSuccess) e = hipMalloc(&t->d_members, t->members_cap * 4);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t->ev, hipEventDisableTiming);
    bool listed = false;
    if (e == hipSuccess) { try { c->committees.push_back(t); listed = true; } catch (...) { } }
    if (!listed) {
        if (t->d_recs) (void)hipFree(t->d_recs);
        if (t->d_members) (void)hipFree(t->d_members);
        if (t->ev) (void)hipEventDestroy(t->ev);
        delete t;
        if (e != hipSuccess) HIPCHK(c, e);
        return MBLS_ERR_DEVICE;
    }
    *out = t; return MBLS_OK;
}
extern "C" void mbls_committees_destroy(mbls_committees* t) {
    if (!t) return;
    if (t->c) {
        mbls_ctx* c = t->c;
        mbls_lock lk(c->mu); (void)hipSetDevice(c->device); (void)hipDeviceSynchronize();
        if (t->d_recs) (void)hipFree(t->d_recs);
        if (t->d_members) (void)hipFree(t->d_members);
        if (t->ev) (void)hipEventDestroy(t->ev);
        for (size_t i = 0; i < c->committees.size(); i++) if (c->committees[i] == t) { c->committees.erase(c->committees.begin() + i); break; }
    }
    delete t;
}
extern "C" uint64_t mbls_committees_count(const mbls_committees* t) { if (!t || !t->c) return 0; mbls_lock lk(t->c->mu); return t->count; }
extern "C" uint32_t mbls_committees_max_members(const mbls_committees* t) { if (!t || !t->c) return 0; mbls_lock lk(t->c->mu); return t->max_members; }
// the two interlocks of a committee stream (mbls_stream.hip; not exported): the count of its calls that have not completed, which mbls_committees_clear consults,
// and the stream's 8 * bits_stride, which mbls_committees_append keeps every committee inside. Binding checks what mbls_stream_create_committee has to refuse, under
// the context's lock, so no append slips between the check and the binding.
extern "C" __attribute__((visibility("hidden"))) void mblsi_committees_stream_calls(mbls_committees* t, long long delta) { if (t) t->stream_calls.fetch_add(delta); }
extern "C" __attribute__((visibility("hidden"))) int mblsi_committees_stream_bind(mbls_ctx* c, mbls_committees* t, uint32_t bits_stride) {
    if (!c || !t) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (t->c != c) ARGFAIL(c, "committee table belongs to another context");
    if (!t->kt || t->kt->c != c) ARGFAIL(c, "the committee table's key table is gone");
    if (bits_stride % 4) ARGFAIL(c, "bits_stride must be a multiple of 4");
    if ((uint64_t)8 * bits_stride < t->max_members) ARGFAIL(c, "bits_stride does not cover the table's largest committee");
    try { t->stream_bits.push_back((uint64_t)8 * bits_stride); } catch (...) { return MBLS_ERR_DEVICE; }
    return MBLS_OK;
}
extern "C" __attribute__((visibility("hidden"))) void mblsi_committees_stream_unbind(mbls_committees* t, uint32_t bits_stride) {
    if (!t || !t->c) return;
    mbls_lock lk(t->c->mu);
    for (size_t i = 0; i < t->stream_bits.size(); i++)
        if (t->stream_bits[i] == (uint64_t)8 * bits_stride) { t->stream_bits.erase(t->stream_bits.begin() + i); break; }
}
extern "C" int mbls_committees_clear(mbls_committees* t) {
    if (!t || !t->c) return MBLS_ERR_ARGUMENT;
    mbls_ctx* c = t->c;
    mbls_lock lk(c->mu);
    if (t->stream_calls.load() > 0) ARGFAIL(c, "committees_clear: a stream bound to the table has calls that have not completed");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());           // every append and verification enqueued over the table
    t->count = 0; t->n_members = 0; t->max_members = 0; t->pending = false; c->ws_pending = false; t->sizes.clear();
    return MBLS_OK;
}
// room for `need` uint32 / `need` records of 40 dwords: new buffer, the device drained on both sides of the copy (keytable_grow's rule)
static int committees_grow(mbls_ctx* c, uint32_t** buf, uint64_t* cap, uint64_t used, uint64_t need, uint64_t unit_dwords) {
    if (need <= *cap) return MBLS_OK;
    const uint64_t ncap = *cap * 2 > need ? *cap * 2 : need;
    uint32_t* nb = nullptr;
    HIPCHK(c, hipMalloc(&nb, ncap * unit_dwords * 4));
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess && used) e = hipMemcpy(nb, *buf, used * unit_dwords * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { (void)hipFree(nb); HIPCHK(c, e); }
    (void)hipFree(*buf); *buf = nb; *cap = ncap;
    return MBLS_OK;
}
extern "C" int mbls_committees_append(mbls_committees* t, const uint32_t* key_idx, const uint32_t* offsets, uint64_t n, uint64_t* first_id) {
    if (!t || !t->c) return MBLS_ERR_ARGUMENT;
    mbls_ctx* c = t->c;
    mbls_lock lk(c->mu);
    if (!n) { if (first_id) *first_id = t->count; return MBLS_OK; }
    if (!key_idx || !offsets) ARGFAIL(c, "null buffer");
    if (!t->kt || t->kt->c != c) ARGFAIL(c, "the committee table's key table is gone");
    if (t->count + n > 0xFFFFFFFFull) ARGFAIL(c, "committee ids are 32-bit");
    uint32_t maxm = t->max_members;
    for (uint64_t i = 0; i < n; i++) {
        if (offsets[i + 1] < offsets[i]) ARGFAIL(c, "offsets must be non-decreasing");
        const uint32_t m = offsets[i + 1] - offsets[i];
        if (m == 0) ARGFAIL(c, "empty committee");
        if (m > MBLS_CMT_MAX_MEMBERS) ARGFAIL(c, "a committee has more than MBLS_COMMITTEE_MAX_MEMBERS members");
        if (m > maxm) maxm = m;
    }
    for (const uint64_t bits : t->stream_bits)
        if (maxm > bits) {          // every later round of that stream would fail the entry's argument check
            snprintf(c->err, sizeof(c->err), "invalid argument: a committee of %u members does not fit the bits_stride of a stream bound to the table (%llu bytes, %llu bits)",
                     maxm, (unsigned long long)(bits / 8), (unsigned long long)bits);
            return MBLS_ERR_ARGUMENT;
        }
    const uint64_t total = (uint64_t)offsets[n] - offsets[0], tsize = t->kt->size;
    const uint32_t* idx = key_idx + offsets[0];
    for (uint64_t j = 0; j < total; j++) if ((uint64_t)idx[j] >= tsize) ARGFAIL(c, "a member index is outside the key table");
    if (t->n_members + total > 0xFFFFFFFFull) ARGFAIL(c, "member positions are 32-bit");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->hs_a;
    int rc = mbls_ctx_reserve(c, n); if (rc) return rc;
    rc = committees_grow(c, &t->d_recs, &t->cap, t->count, t->count + n, MBLS_CMT_REC_DWORDS); if (rc) return rc;
    rc = committees_grow(c, &t->d_members, &t->members_cap, t->n_members, t->n_members + total, 1); if (rc) return rc;
    // the offsets as the kernels want them: relative to the append's first member
    std::vector<uint32_t> rel;
    try { rel.resize(n + 1); t->sizes.reserve(t->count + n); } catch (...) { return MBLS_ERR_DEVICE; }
    for (uint64_t i = 0; i <= n; i++) rel[i] = offsets[i] - offsets[0];
    sbuf doff(c, 3);
    HIPCHK(c, doff.up(rel.data(), 4 * (n + 1)));
    rc = ws_acquire(c, s); if (rc) return rc;
    rc = table_acquire(c, t->kt, s); if (rc) return rc;              // pending appends to the key table
    rc = committees_acquire(c, t, s); if (rc) return rc;
    uint32_t* const d_new = t->d_members + t->n_members;
    HIPCHK(c, hipMemcpyAsync(d_new, idx, 4 * total, hipMemcpyHostToDevice, s));
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    HIPCHK(c, hipMemsetAsync(c->d_status, 0, 4 * n, s));
    hipLaunchKernelGGL(k_aggregate_indexed_d, dim3(nblk(n)), dim3(WG), 0, s, ws, (const uint32_t*)t->kt->d_recs, t->kt->size, (const uint32_t*)d_new,
                       (const uint32_t*)doff.as<uint32_t>(), 0u, MBLS_MODE_VERIFY, c->d_status, n);
    hipLaunchKernelGGL(k_cmt_build, dim3(nblk(n)), dim3(WG), 0, s, ws, (const uint32_t*)c->d_status, (const uint32_t*)doff.as<uint32_t>(), t->n_members,
                       t->d_recs + t->count * MBLS_CMT_REC_DWORDS, n);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(t->ev, s)); t->ev_stream = s; t->pending = true;
    // the staged offsets and the caller's indices are read until the kernels have run
    HIPCHK(c, hipStreamSynchronize(s));
    c->ws_pending = false; t->pending = false;
    if (first_id) *first_id = t->count;
    for (uint64_t i = 0; i < n; i++) t->sizes.push_back(offsets[i + 1] - offsets[i]);       // (reserved above: nothing throws here)
    t->count += n; t->n_members += total; t->max_members = maxm;
    return MBLS_OK;
}
extern "C" int mbls_committees_get(mbls_committees* t, uint64_t id, uint8_t* sum96, uint32_t* n_members, uint32_t* eligible) {
    if (!t || !t->c) return MBLS_ERR_ARGUMENT;
    mbls_ctx* c = t->c;
    mbls_lock lk(c->mu);
    if (id >= t->count) ARGFAIL(c, "committees_get: no such committee");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->hs_a;
    sbuf dout(c, 0); HIPCHK(c, dout.alloc(96));
    int rc = committees_acquire(c, t, s); if (rc) return rc;
    const uint32_t* rec = t->d_recs + id * MBLS_CMT_REC_DWORDS;
    hipLaunchKernelGGL(k_cmt_export, dim3(1), dim3(WG), 0, s, rec, dout.as<uint8_t>());
    HIPCHK(c, hipGetLastError());
    uint32_t head[4];
    HIPCHK(c, hipMemcpyAsync(head, rec, sizeof(head), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (sum96) HIPCHK(c, dout.down(sum96, 96));
    if (n_members) *n_members = head[1];
    if (eligible) *eligible = head[2];
    return MBLS_OK;
}
// the key source of a _committee entry: the table and its key table at the sizes they have now (the caller holds the context's lock)
static int keys_of_committees(mbls_ctx* c, const mbls_committees* t, const uint32_t* d_cmt_idx, const uint8_t* d_bits, uint32_t bits_stride, bool device_bits, keysrc* ks) {
    if (t->c != c) ARGFAIL(c, "committee table belongs to another context");
    if (!t->kt || t->kt->c != c) ARGFAIL(c, "the committee table's key table is gone");
    if (bits_stride % 4) ARGFAIL(c, "bits_stride must be a multiple of 4");
    if ((uint64_t)8 * bits_stride < t->max_members) ARGFAIL(c, "bits_stride does not cover the table's largest committee");
    if (device_bits && (((uintptr_t)d_bits) & 3u)) ARGFAIL(c, "d_bits must be 4-byte aligned");
    keysrc kt; const int rk = keys_of_table(c, t->kt, nullptr, nullptr, &kt); if (rk) return rk;
    *ks = keys_committee(kt, t->d_recs, t->count, t->d_members, t->max_members, d_cmt_idx, d_bits, bits_stride, t);
    return MBLS_OK;
}
// a committee call on the device: the table read at the sizes it has now, then the one way into the pipeline (verify_device reserves the scratch of the plan)
static int verify_committee_device(mbls_ctx* c, const mbls_committees* t, const uint8_t* d_sigs, msgsrc ms, const mbls_msgtable* mt, const uint32_t* d_cmt_idx,
                                   const uint8_t* d_bits, uint32_t bits_stride, uint64_t n, uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, hipStream_t s) {
    keysrc ks; const int rk = keys_of_committees(c, t, d_cmt_idx, d_bits, bits_stride, true, &ks); if (rk) return rk;
    if (n == 0) return MBLS_OK;
    if (!d_cmt_idx || !d_bits) ARGFAIL(c, "null buffer");
    return verify_device(c, batch{d_sigs, ms, ks, n, 0, MBLS_MODE_FAST_AGGREGATE, d_results, d_bitmap, d_status}, mt, s);
}
extern "C" int mbls_fast_aggregate_verify_batch_committee_device(mbls_ctx* c, const mbls_committees* t, const uint8_t* d_sigs, const uint8_t* d_msgs, uint32_t msg_len,
        const uint64_t* d_moff, const uint32_t* d_cmt_idx, const uint8_t* d_bits, uint32_t bits_stride, uint64_t n, uint8_t* d_results, uint64_t* d_bitmap,
        uint32_t* d_status, void* stream) {
    if (!c || !t) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    return verify_committee_device(c, t, d_sigs, msgs_per_item(d_msgs, msg_len, d_moff), nullptr, d_cmt_idx, d_bits, bits_stride, n, d_results, d_bitmap, d_status,
                                   (hipStream_t)stream);
}
extern "C" int mbls_fast_aggregate_verify_batch_committee_msgtable_device(mbls_ctx* c, const mbls_committees* t, const uint8_t* d_sigs, const mbls_msgtable* mt,
        const uint32_t* d_msg_idx, const uint32_t* d_cmt_idx, const uint8_t* d_bits, uint32_t bits_stride, uint64_t n, uint8_t* d_results, uint64_t* d_bitmap,
        uint32_t* d_status, void* stream) {
    if (!c || !t || !mt) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    return verify_committee_device(c, t, d_sigs, msgs_in_table(d_msg_idx), mt, d_cmt_idx, d_bits, bits_stride, n, d_results, d_bitmap, d_status, (hipStream_t)stream);
}
// the host forms: verify_host with the committee description in place of keys
extern "C" int mbls_fast_aggregate_verify_batch_committee(mbls_ctx* c, const mbls_committees* t, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len,
        const uint64_t* moff, const uint32_t* cmt_idx, const uint8_t* bits, uint32_t bits_stride, uint64_t n, uint8_t* results, uint32_t* status) {
    if (!c || !t) return MBLS_ERR_ARGUMENT;
    const host_committees hc = {t, cmt_idx, bits, bits_stride};
    return verify_host(c, sigs, msgs_per_item(msgs, msg_len, moff), nullptr, nullptr, MBLS_PK_UNCOMPRESSED, nullptr, nullptr, nullptr, n, 0, MBLS_MODE_FAST_AGGREGATE, results, status, &hc);
}
extern "C" int mbls_fast_aggregate_verify_batch_committee_msgtable(mbls_ctx* c, const mbls_committees* t, const uint8_t* sigs, const mbls_msgtable* mt,
        const uint32_t* msg_idx, const uint32_t* cmt_idx, const uint8_t* bits, uint32_t bits_stride, uint64_t n, uint8_t* results, uint32_t* status) {
    if (!c || !t || !mt) return MBLS_ERR_ARGUMENT;
    const host_committees hc = {t, cmt_idx, bits, bits_stride};
    return verify_host(c, sigs, msgs_in_table(msg_idx), mt, nullptr, MBLS_PK_UNCOMPRESSED, nullptr, nullptr, nullptr, n, 0, MBLS_MODE_FAST_AGGREGATE, results, status, &hc);
}

// ---- committee spans (include/mbls.h, "committee spans"; arithmetic: mbls_cms.h, device bodies: mbls_cms_lanes.h): the committee entries with, per item, a range of
// committee ids and one bitfield over their concatenated members. The key source is the committee form's with the span fields; the pass launches k_cms_expand and
// k_aggregate_cms_d where the committee form launches its two kernels, and verify_device reserves the span scratch for the plan's extent.
static int keys_of_committee_span(mbls_ctx* c, const mbls_committees* t, const uint32_t* d_cmt_ids, uint64_t n_cmt_ids, const uint32_t* d_cmt_off, const uint8_t* d_bits,
                                  uint32_t bits_stride, bool device_bits, keysrc* ks) {
    if (t->c != c) ARGFAIL(c, "committee table belongs to another context");
    if (!t->kt || t->kt->c != c) ARGFAIL(c, "the committee table's key table is gone");
    if (bits_stride % 4) ARGFAIL(c, "bits_stride must be a multiple of 4");
    if (n_cmt_ids > 0xFFFFFFFFull) ARGFAIL(c, "span offsets are 32-bit");
    if (device_bits && (((uintptr_t)d_bits) & 3u)) ARGFAIL(c, "d_bits must be 4-byte aligned");
    keysrc kt; const int rk = keys_of_table(c, t->kt, nullptr, nullptr, &kt); if (rk) return rk;
    *ks = keys_committee_span(kt, t->d_recs, t->count, t->d_members, t->max_members, d_cmt_ids, n_cmt_ids, d_cmt_off, d_bits, bits_stride, t);
    return MBLS_OK;
}
// the host entries' statement of "malformed": what wave_cms_expand rejects per item refuses the whole call here (the caller holds the context's lock)
static int committee_span_items_ok(mbls_ctx* c, const host_committees& hc, uint64_t n) {
    if (!hc.cmt_off || (hc.n_cmt_ids && !hc.cmt_ids) || (hc.bits_stride && !hc.bits)) ARGFAIL(c, "null buffer");
    for (uint64_t i = 0; i < n; i++) {
        uint32_t q = 0;
        if (!cms_range_ok(hc.cmt_off[i], hc.cmt_off[i + 1], hc.n_cmt_ids, &q)) ARGFAIL(c, "cmt_off must be non-decreasing, inside cmt_ids, at most MBLS_SPAN_MAX_COMMITTEES ids per item");
        uint64_t M = 0;
        for (uint32_t u = 0; u < q; u++) {
            const uint32_t cid = hc.cmt_ids[(uint64_t)hc.cmt_off[i] + u];
            if ((uint64_t)cid >= hc.t->count) ARGFAIL(c, "cmt_ids names no committee of the table");
            M += hc.t->sizes[cid];
        }
        if (!cms_field_ok(M, hc.bits_stride)) ARGFAIL(c, "bits_stride does not cover an item's committees");
    }
    return MBLS_OK;
}
static int verify_committee_span_device(mbls_ctx* c, const mbls_committees* t, const uint8_t* d_sigs, msgsrc ms, const mbls_msgtable* mt, const uint32_t* d_cmt_ids,
                                        uint64_t n_cmt_ids, const uint32_t* d_cmt_off, const uint8_t* d_bits, uint32_t bits_stride, uint64_t n, uint8_t* d_results,
                                        uint64_t* d_bitmap, uint32_t* d_status, hipStream_t s) {
    keysrc ks; const int rk = keys_of_committee_span(c, t, d_cmt_ids, n_cmt_ids, d_cmt_off, d_bits, bits_stride, true, &ks); if (rk) return rk;
    if (n == 0) return MBLS_OK;
    if (!d_cmt_off || (n_cmt_ids && !d_cmt_ids) || (bits_stride && !d_bits)) ARGFAIL(c, "null buffer");
    return verify_device(c, batch{d_sigs, ms, ks, n, 0, MBLS_MODE_FAST_AGGREGATE, d_results, d_bitmap, d_status}, mt, s);
}
extern "C" int mbls_fast_aggregate_verify_batch_committee_span_device(mbls_ctx* c, const mbls_committees* t, const uint8_t* d_sigs, const uint8_t* d_msgs, uint32_t msg_len,
        const uint64_t* d_moff, const uint32_t* d_cmt_ids, uint64_t n_cmt_ids, const uint32_t* d_cmt_off, const uint8_t* d_bits, uint32_t bits_stride, uint64_t n,
        uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream) {
    if (!c || !t) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    return verify_committee_span_device(c, t, d_sigs, msgs_per_item(d_msgs, msg_len, d_moff), nullptr, d_cmt_ids, n_cmt_ids, d_cmt_off, d_bits, bits_stride, n, d_results,
                                        d_bitmap, d_status, (hipStream_t)stream);
}
extern "C" int mbls_fast_aggregate_verify_batch_committee_span_msgtable_device(mbls_ctx* c, const mbls_committees* t, const uint8_t* d_sigs, const mbls_msgtable* mt,
        const uint32_t* d_msg_idx, const uint32_t* d_cmt_ids, uint64_t n_cmt_ids, const uint32_t* d_cmt_off, const uint8_t* d_bits, uint32_t bits_stride, uint64_t n,
        uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream) {
    if (!c || !t || !mt) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    return verify_committee_span_device(c, t, d_sigs, msgs_in_table(d_msg_idx), mt, d_cmt_ids, n_cmt_ids, d_cmt_off, d_bits, bits_stride, n, d_results, d_bitmap, d_status,
                                        (hipStream_t)stream);
}
// the host forms: verify_host with the span description in place of keys
extern "C" int mbls_fast_aggregate_verify_batch_committee_span(mbls_ctx* c, const mbls_committees* t, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len,
        const uint64_t* moff, const uint32_t* cmt_ids, uint64_t n_cmt_ids, const uint32_t* cmt_off, const uint8_t* bits, uint32_t bits_stride, uint64_t n,
        uint8_t* results, uint32_t* status) {
    if (!c || !t) return MBLS_ERR_ARGUMENT;
    host_committees hc = {t, nullptr, bits, bits_stride}; hc.span = true; hc.cmt_ids = cmt_ids; hc.n_cmt_ids = n_cmt_ids; hc.cmt_off = cmt_off;
    return verify_host(c, sigs, msgs_per_item(msgs, msg_len, moff), nullptr, nullptr, MBLS_PK_UNCOMPRESSED, nullptr, nullptr, nullptr, n, 0, MBLS_MODE_FAST_AGGREGATE, results, status, &hc);
}
extern "C" int mbls_fast_aggregate_verify_batch_committee_span_msgtable(mbls_ctx* c, const mbls_committees* t, const uint8_t* sigs, const mbls_msgtable* mt,
        const uint32_t* msg_idx, const uint32_t* cmt_ids, uint64_t n_cmt_ids, const uint32_t* cmt_off, const uint8_t* bits, uint32_t bits_stride, uint64_t n,
        uint8_t* results, uint32_t* status) {
    if (!c || !t || !mt) return MBLS_ERR_ARGUMENT;
    host_committees hc = {t, nullptr, bits, bits_stride}; hc.span = true; hc.cmt_ids = cmt_ids; hc.n_cmt_ids = n_cmt_ids; hc.cmt_off = cmt_off;
    return verify_host(c, sigs, msgs_in_table(msg_idx), mt, nullptr, MBLS_PK_UNCOMPRESSED, nullptr, nullptr, nullptr, n, 0, MBLS_MODE_FAST_AGGREGATE, results, status, &hc);
}

// ---- batch helpers
extern "C" int mbls_pk_decode_batch(mbls_ctx* c, const uint8_t* in, int fmt, int validate, uint64_t n, uint8_t* out96, uint8_t* errs) {
    if (!c || !in || !out96 || !errs || (fmt != 0 && fmt != 1)) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (!n) return MBLS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    sbuf di(c, 0), dout(c, 1), de(c, 2); HIPCHK(c, di.up(in, (fmt ? 96 : 48) * n)); HIPCHK(c, dout.alloc(96 * n)); HIPCHK(c, de.alloc(n));
    hipLaunchKernelGGL(k_g1_decode, dim3(nblk(n)), dim3(WG), 0, c->hs_a, di.as<uint8_t>(), fmt, validate, n, dout.as<uint8_t>(), de.as<uint8_t>());
    HIPCHK(c, hipStreamSynchronize(c->hs_a)); HIPCHK(c, dout.down(out96, 96 * n)); HIPCHK(c, de.down(errs, n));
    for (uint64_t i = 0; i < n; i++) errs[i] = (uint8_t)map_dec_err_g1(errs[i]);
    return MBLS_OK;
}
extern "C" int mbls_pk_compress_batch(mbls_ctx* c, const uint8_t* in96, uint64_t n, uint8_t* out48, uint8_t* errs) {
    if (!c || !in96 || !out48 || !errs) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (!n) return MBLS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    sbuf di(c, 0), dout(c, 1), de(c, 2); HIPCHK(c, di.up(in96, 96 * n)); HIPCHK(c, dout.alloc(48 * n)); HIPCHK(c, de.alloc(n));
    hipLaunchKernelGGL(k_g1_compress, dim3(nblk(n)), dim3(WG), 0, c->hs_a, di.as<uint8_t>(), n, dout.as<uint8_t>(), de.as<uint8_t>());
    HIPCHK(c, hipStreamSynchronize(c->hs_a)); HIPCHK(c, dout.down(out48, 48 * n)); HIPCHK(c, de.down(errs, n));
    for (uint64_t i = 0; i < n; i++) errs[i] = (uint8_t)map_dec_err_g1(errs[i]);
    return MBLS_OK;
}
extern "C" int mbls_sig_check_batch(mbls_ctx* c, const uint8_t* in96, uint64_t n, uint8_t* errs, uint8_t* in_g2) {
    if (!c || !in96 || !errs) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (!n) return MBLS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    sbuf di(c, 0), de(c, 1), dg(c, 2); HIPCHK(c, di.up(in96, 96 * n)); HIPCHK(c, de.alloc(n)); if (in_g2) HIPCHK(c, dg.alloc(n));
    int rc = mbls_ctx_reserve(c, n); if (rc) return rc;               // the subgroup routine works on the items' workspace slots
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    rc = ws_acquire(c, c->hs_a); if (rc) return rc;
    hipLaunchKernelGGL(k_g2_check, dim3(nblk(n)), dim3(WG), 0, c->hs_a, ws, di.as<uint8_t>(), n, de.as<uint8_t>(), in_g2 ? dg.as<uint8_t>() : (uint8_t*)nullptr);
    HIPCHK(c, hipStreamSynchronize(c->hs_a)); c->ws_pending = false; HIPCHK(c, de.down(errs, n)); if (in_g2) HIPCHK(c, dg.down(in_g2, n));
    for (uint64_t i = 0; i < n; i++) errs[i] = (uint8_t)map_dec_err_g2(errs[i]);
    return MBLS_OK;
}
static void g2_tree_levels(mbls_ctx* c, mbls_ws ws, uint64_t m, int levels, hipStream_t s);
// Secret-dependent words do not outlive the call that made them: workspace slots [slot_lo, slot_hi) of items 0..m-1 are zeroed on the
// stream (word-major layout: one row of `stride` items per word, so this is a 2-D fill of m items x 12 (slot_hi - slot_lo) rows).
// NOTE the signing / key-derivation kernels are NOT constant-time: k_aggregate_indexed_d gathers table records at secret-dependent
// addresses and the window digits of k_sign_blind select per-lane records (include/mbls.h says so at mbls_sign_batch).
static hipError_t ws_wipe(mbls_ctx* c, int slot_lo, int slot_hi, uint64_t m, hipStream_t s) {
    return hipMemset2DAsync(c->d_w + (size_t)slot_lo * 12 * c->cap, c->cap * 4, 0, m * 4, (size_t)(slot_hi - slot_lo) * 12, s);
}
// the error path of the host entries: the device entry refused or failed, the staged secret keys go all the same. What the device entry said stays the call's
// answer (the context's error text included), so nothing here is checked: after a failure of the runtime itself the fill may fail as well (include/mbls.h).
static void staged_keys_wipe(mbls_ctx* c, void* d_keys, size_t bytes) {
    (void)hipMemsetAsync(d_keys, 0, bytes, c->hs_a); (void)hipStreamSynchronize(c->hs_a);
}
// [sk] H(msg) for n (secret key, message) pairs: the pipeline's message phase, the four-lane windowed multiplication (k_sign_blind), two
// levels of the G2 sum tree, compression -- in chunks of MBLS_SIGN_CHUNK signatures (four workspace items each). Enqueues only.
#define MBLS_SIGN_CHUNK 65536ull
extern "C" int mbls_sign_batch_device(mbls_ctx* c, const uint8_t* d_sks, const uint8_t* d_msgs, uint32_t msg_len, uint64_t n, uint8_t* d_sigs, void* stream) {
    if (!c || !d_sks || !d_sigs || (!d_msgs && msg_len)) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (!n) return MBLS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const uint64_t chunk = n < MBLS_SIGN_CHUNK ? n : MBLS_SIGN_CHUNK;
    int rc = mbls_ctx_reserve(c, 4 * chunk); if (rc) return rc;
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    rc = ws_acquire(c, s); if (rc) return rc;
    for (uint64_t lo = 0; lo < n; lo += chunk) {
        const uint64_t m = n - lo < chunk ? n - lo : chunk;
        HIPCHK(c, hipMemsetAsync(c->d_status, 0, 4 * m, s));
        launch_hash(c, ws, d_msgs + (uint64_t)msg_len * lo, msg_len, nullptr, c->d_status, m, s);
        hipLaunchKernelGGL(k_sign_blind, dim3(nblk(4 * m)), dim3(WG), 0, s, ws, d_sks + 32 * lo, m, c->secret_ops_fast ? 0 : 1);
        g2_tree_levels(c, ws, 4 * m, 2, s);
        hipLaunchKernelGGL(k_s_export, dim3(nblk(m)), dim3(WG), 0, s, ws, m, d_sigs + 96 * lo);
    }
    HIPCHK(c, hipGetLastError());
    // the four partial products [a_j] psi^j(H) (slots SIG, S) and their window tables (KREC..) are functions of the secret key
    HIPCHK(c, ws_wipe(c, MBLS_SLOT_SIG, MBLS_SLOT_SIG + 4, 4 * chunk, s));
    HIPCHK(c, ws_wipe(c, MBLS_SLOT_S, MBLS_SLOT_S + 6, 4 * chunk, s));
    HIPCHK(c, ws_wipe(c, MBLS_SLOT_KREC, MBLS_SLOT_KREC + 48 + 6, 4 * chunk, s));        // the tables and (constant-time form) the record each window selected: 49..102
    // a tree level on lanes (k_g2_tree_d, above MBLS_COOP_TREE_PAIRS pairs) parks the partner's running sum -- [a_2] psi^2(H), [a_3] psi^3(H), then
    // [a_1] psi(H) + [a_3] psi^3(H) -- in the staging slots of the lane's own item (tools/gen_tower_d.py prog_g2_tree_start): 43..48
    HIPCHK(c, ws_wipe(c, MBLS_SLOT_G2TMP, MBLS_SLOT_G2TMP + 6, 4 * chunk, s));
    return ws_release(c, s);
}
extern "C" int mbls_sign_batch(mbls_ctx* c, const uint8_t* sks, const uint8_t* msgs, uint32_t msg_len, uint64_t n, uint8_t* sigs) {
    if (!c || !sks || !sigs || (!msgs && msg_len)) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (!n) return MBLS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    // the keys go up LAST: nothing between their upload and the device entry can fail
    sbuf dk(c, 0), dm(c, 1), dout(c, 2); HIPCHK(c, dm.up(msgs, (size_t)msg_len * n)); HIPCHK(c, dout.alloc(96 * n)); HIPCHK(c, dk.up(sks, 32 * n));
    int rc = mbls_sign_batch_device(c, dk.as<uint8_t>(), dm.as<uint8_t>(), msg_len, n, dout.as<uint8_t>(), c->hs_a);
    if (rc) { staged_keys_wipe(c, dk.p, 32 * n); return rc; }
    HIPCHK(c, hipMemsetAsync(dk.p, 0, 32 * n, c->hs_a));                  // the staged secret keys
    HIPCHK(c, hipStreamSynchronize(c->hs_a)); HIPCHK(c, dout.down(sigs, 96 * n)); return MBLS_OK;
}
// the fixed table of sk -> pk: the 1 024 multiples come from the compiled ladder (k_sk_to_pk) once per context
static int ensure_gtab(mbls_ctx* c) {
    if (c->d_gtab) return MBLS_OK;
    std::vector<uint8_t> sc(32 * 1024, 0);
    for (int j = 0; j < 64; j++) for (int d = 0; d < 16; d++) sc[32 * (16 * j + d) + 31 - (j >> 1)] = (uint8_t)(d << (4 * (j & 1)));
    HIPCHK(c, hipDeviceSynchronize());       // once per context: nothing in flight may still be reading the staging buffers used here
    sbuf dk(c, 7), dp(c, 8), de(c, 9);      // not the staging slots of the host entries that call this with their inputs already uploaded
    HIPCHK(c, dk.up(sc.data(), sc.size())); HIPCHK(c, dp.alloc(96 * 1024)); HIPCHK(c, de.alloc(1024));
    uint32_t* tab = nullptr; HIPCHK(c, hipMalloc(&tab, 1024 * MBLS_KEYREC_DWORDS * 4));
    hipLaunchKernelGGL(k_sk_to_pk, dim3(nblk(1024)), dim3(WG), 0, c->hs_a, dk.as<uint8_t>(), MBLS_PK_UNCOMPRESSED, (uint64_t)1024, dp.as<uint8_t>());
    hipLaunchKernelGGL(k_keytable_append, dim3(nblk(1024)), dim3(WG), 0, c->hs_a, dp.as<uint8_t>(), MBLS_PK_UNCOMPRESSED, 0, (uint64_t)1024, tab, de.as<uint8_t>());
    hipError_t e = hipStreamSynchronize(c->hs_a);
    std::vector<uint8_t> errs(1024, 1);
    if (e == hipSuccess) e = de.down(errs.data(), 1024);
    bool ok = e == hipSuccess;
    for (int t = 0; ok && t < 1024; t++) ok = errs[t] == 0;
    if (!ok) { (void)hipFree(tab); snprintf(c->err, sizeof(c->err), "building the generator table failed"); return MBLS_ERR_DEVICE; }
    c->d_gtab = tab; return MBLS_OK;
}
#define MBLS_SKPK_CHUNK 131072ull
#define MBLS_SKPK_CT_CHUNK 32768ull          /* constant-time form: 64 selected records of 128 bytes per key are staged (256 MB per chunk) */
extern "C" int mbls_sk_to_pk_batch_device(mbls_ctx* c, const uint8_t* d_sks, int fmt, uint64_t n, uint8_t* d_pks, void* stream) {
    if (!c || !d_sks || !d_pks || (fmt != 0 && fmt != 1)) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (!n) return MBLS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    int rc = ensure_gtab(c); if (rc) return rc;
    const bool ct = !c->secret_ops_fast;
    const uint64_t cmax = ct ? MBLS_SKPK_CT_CHUNK : MBLS_SKPK_CHUNK;
    const uint64_t chunk = n < cmax ? n : cmax;
    rc = mbls_ctx_reserve(c, chunk); if (rc) return rc;
    if (c->skidx_cap < chunk) {
        if (c->d_skidx) { (void)hipFree(c->d_skidx); c->d_skidx = nullptr; c->skidx_cap = 0; }
        HIPCHK(c, hipMalloc(&c->d_skidx, chunk * 64 * 4)); c->skidx_cap = chunk;
    }
    if (ct && c->sksel_cap < chunk) {
        if (c->d_sksel) { (void)hipFree(c->d_sksel); c->d_sksel = nullptr; c->sksel_cap = 0; }
        HIPCHK(c, hipMalloc(&c->d_sksel, chunk * 64 * MBLS_KEYREC_DWORDS * 4)); c->sksel_cap = chunk;
    }
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    rc = ws_acquire(c, s); if (rc) return rc;
    for (uint64_t lo = 0; lo < n; lo += chunk) {
        const uint64_t m = n - lo < chunk ? n - lo : chunk;
        HIPCHK(c, hipMemsetAsync(c->d_status, 0, 4 * m, s));
        if (ct) {
            // the records are chosen by scan + selection (k_sk_select), the key sum then walks sel[64 i + j]: public indices, public addresses
            hipLaunchKernelGGL(k_sk_select, dim3(nblk(64 * m)), dim3(WG), 0, s, d_sks + 32 * lo, m, (const uint32_t*)c->d_gtab, c->d_sksel, c->d_skidx);
            hipLaunchKernelGGL(k_aggregate_indexed_d, dim3(nblk(m)), dim3(WG), 0, s, ws, (const uint32_t*)c->d_sksel, (uint64_t)(64 * m), (const uint32_t*)c->d_skidx,
                               (const uint32_t*)nullptr, 64u, MBLS_MODE_VERIFY, c->d_status, m);
        } else {
            hipLaunchKernelGGL(k_sk_digits, dim3(nblk(m)), dim3(WG), 0, s, d_sks + 32 * lo, m, c->d_skidx);
            hipLaunchKernelGGL(k_aggregate_indexed_d, dim3(nblk(m)), dim3(WG), 0, s, ws, (const uint32_t*)c->d_gtab, (uint64_t)1024, (const uint32_t*)c->d_skidx,
                               (const uint32_t*)nullptr, 64u, MBLS_MODE_VERIFY, c->d_status, m);
        }
        hipLaunchKernelGGL(k_apk_export_fmt, dim3(nblk(m)), dim3(WG), 0, s, ws, m, fmt, d_pks + (uint64_t)(fmt ? 96 : 48) * lo);
    }
    HIPCHK(c, hipGetLastError());
    if (ct) HIPCHK(c, hipMemsetAsync(c->d_sksel, 0, chunk * 64 * MBLS_KEYREC_DWORDS * 4, s));            // the selected multiples are functions of the keys
    else HIPCHK(c, hipMemsetAsync(c->d_skidx, 0, chunk * 64 * 4, s));            // the hexadecimal digits of the secret keys
    // the key sum leaves [sk] G1 (Jacobian) in slot APK of the items, and in their status words MBLS_ST_PK_INFINITY for every key with a hexadecimal digit 0 (record
    // 16 j of the table is the point at infinity): which keys have NO such digit is a function of the keys
    HIPCHK(c, ws_wipe(c, MBLS_SLOT_APK, MBLS_SLOT_APK + 3, chunk, s));
    HIPCHK(c, hipMemsetAsync(c->d_status, 0, 4 * chunk, s));
    return ws_release(c, s);
}
// 1: table lookups that depend on a secret key (the window tables of signing, the generator table of sk -> pk) go back to the faster forms that read ONE record
// at an address computed from the key's digits -- for building test and bench inputs from throw-away keys only. 0 (default): scan + selection.
extern "C" int mbls_ctx_set_secret_ops(mbls_ctx* c, int variable_time) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu); c->secret_ops_fast = variable_time != 0; return MBLS_OK;
}
extern "C" int mbls_sk_to_pk_batch(mbls_ctx* c, const uint8_t* sks, int fmt, uint64_t n, uint8_t* pks) {
    if (!c || !sks || !pks || (fmt != 0 && fmt != 1)) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (!n) return MBLS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    sbuf dk(c, 0), dout(c, 1); HIPCHK(c, dout.alloc((fmt ? 96 : 48) * n)); HIPCHK(c, dk.up(sks, 32 * n));             // the keys last, as in mbls_sign_batch
    int rc = mbls_sk_to_pk_batch_device(c, dk.as<uint8_t>(), fmt, n, dout.as<uint8_t>(), c->hs_a);
    if (rc) { staged_keys_wipe(c, dk.p, 32 * n); return rc; }
    HIPCHK(c, hipMemsetAsync(dk.p, 0, 32 * n, c->hs_a));                  // the staged secret keys
    HIPCHK(c, hipStreamSynchronize(c->hs_a)); HIPCHK(c, dout.down(pks, (fmt ? 96 : 48) * n)); return MBLS_OK;
}
extern "C" int mbls_hash_to_g2_batch_mode(mbls_ctx* c, const uint8_t* msgs, uint32_t msg_len, uint64_t n, uint8_t* out96, int mode);
extern "C" int mbls_hash_to_g2_batch(mbls_ctx* c, const uint8_t* msgs, uint32_t msg_len, uint64_t n, uint8_t* out96) {
    return mbls_hash_to_g2_batch_mode(c, msgs, msg_len, n, out96, 0);
}
extern "C" int mbls_hash_to_g2_batch_mode(mbls_ctx* c, const uint8_t* msgs, uint32_t msg_len, uint64_t n, uint8_t* out96, int mode) {
    if (!c || !out96 || (!msgs && msg_len) || mode < 0 || mode > 3) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (!n) return MBLS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    sbuf dm(c, 0), dout(c, 1); HIPCHK(c, dm.up(msgs, (size_t)msg_len * n)); HIPCHK(c, dout.alloc(96 * n));
    {                     // the pipeline's message phase (mode 0: the form a batch of this size takes by itself; mode 1: one lane per item, the generated routine;
                          // mode 2: one wave per item, program hashg2; mode 3: two lanes per item), then its H
        const bool pair0 = mode == 0 && 2 * n <= c->round_items;
        int rc = mbls_ctx_reserve(c, (mode == 3 || pair0) ? 2 * n : n); if (rc) return rc;
        mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
        rc = ws_acquire(c, c->hs_a); if (rc) return rc;
        HIPCHK(c, hipMemsetAsync(c->d_status, 0, 4 * n, c->hs_a));
        // the form is named, not routed: mode 1 one lane per item, mode 2 one wave per item (four items per wave above the packing limit), mode 3 two lanes per item
        launch_hash(c, ws, dm.as<uint8_t>(), msg_len, nullptr, c->d_status, n, c->hs_a, mode == 3 || pair0,
                    mode == 0 ? HASH_FORM_AUTO : mode == 1 ? HASH_FORM_LANE : mode == 2 ? HASH_FORM_WAVE : HASH_FORM_PAIR);
        hipLaunchKernelGGL(k_h_export, dim3(nblk(n)), dim3(WG), 0, c->hs_a, ws, n, dout.as<uint8_t>());
    }
    HIPCHK(c, hipStreamSynchronize(c->hs_a)); c->ws_pending = false; HIPCHK(c, dout.down(out96, 96 * n)); return MBLS_OK;
}
// the probes below take canonical 48-byte big-endian field elements: every one must be below p
static const uint8_t MBLS_P_BE[48] = {0x1a, 0x01, 0x11, 0xea, 0x39, 0x7f, 0xe6, 0x9a, 0x4b, 0x1b, 0xa7, 0xb6, 0x43, 0x4b, 0xac, 0xd7, 0x64, 0x77, 0x4b, 0x84, 0xf3, 0x85, 0x12, 0xbf,
                                      0x67, 0x30, 0xd2, 0xa0, 0xf6, 0xb0, 0xf6, 0x24, 0x1e, 0xab, 0xff, 0xfe, 0xb1, 0x53, 0xff, 0xff, 0xb9, 0xfe, 0xff, 0xff, 0xff, 0xff, 0xaa, 0xab};
static bool all_below_p(const uint8_t* v48, uint64_t count) {
    for (uint64_t j = 0; j < count; j++) if (memcmp(v48 + 48 * j, MBLS_P_BE, 48) >= 0) return false;
    return true;
}
// test probe: the message phase after hash_to_field on the caller's field elements (include/mbls.h). The import kernel stands in for hash_fields_to_ws; from
// there every mode runs what launch_hash runs for that form -- the same generated routines and wave programs, the packing limit obeyed -- and k_h_export.
extern "C" int mbls_map_to_g2_probe(mbls_ctx* c, const uint8_t* u192, uint64_t n, uint8_t* out96, int mode) {
    if (!c || !out96 || (!u192 && n) || mode < 0 || mode > 3) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (!n) return MBLS_OK;
    if (!all_below_p(u192, 4 * n)) ARGFAIL(c, "a field element is not below p");
    HIPCHK(c, hipSetDevice(c->device));
    sbuf du(c, 0), dout(c, 1); HIPCHK(c, du.up(u192, 192 * n)); HIPCHK(c, dout.alloc(96 * n));
    const uint64_t lanes = mode == 3 ? 2 * n : n;
    int rc = mbls_ctx_reserve(c, lanes); if (rc) return rc;
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    hipStream_t s = c->hs_a;
    rc = ws_acquire(c, s); if (rc) return rc;
    hipLaunchKernelGGL(k_map_import, dim3(nblk(lanes)), dim3(WG), 0, s, ws, du.as<uint8_t>(), n, mode == 3 ? 1 : 0);
    if (mode == 0)
        hipLaunchKernelGGL(k_map_body, dim3(nblk(n)), dim3(WG), 0, s, ws, n);
    else if (mode == 1)
        hipLaunchKernelGGL(k_map_lane, dim3(nblk(n)), dim3(WG), 0, s, ws, n);
    else if (mode == 2)
        coop_run(c, n > c->coop_hash_pack_min_items ? COOP_HASHG2X4 : COOP_HASHG2, ws, (uint64_t)0, (uint64_t)1, (uint64_t)0, n, (uint32_t*)nullptr, (uint8_t*)nullptr, COOP_RES_ITEM, s);
    else {
        hipLaunchKernelGGL(k_map_pair, dim3(nblk(2 * n)), dim3(WG), 0, s, ws, n);
        hipLaunchKernelGGL(k_h_compact_a, dim3(nblk(n)), dim3(WG), 0, s, ws, n);
        hipLaunchKernelGGL(k_h_compact_b, dim3(nblk(n)), dim3(WG), 0, s, ws, n);
    }
    hipLaunchKernelGGL(k_h_export, dim3(nblk(n)), dim3(WG), 0, s, ws, n, dout.as<uint8_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s)); c->ws_pending = false; HIPCHK(c, dout.down(out96, 96 * n)); return MBLS_OK;
}
// Test probes of the pairing (mbls_miller_probe, mbls_final_exp_probe; include/mbls.h): the caller's operands go into the workspace slots the phase kernels fill,
// the form the mode names runs EXACTLY what the pipeline launches for it -- the same kernels, generated routines and wave programs, nothing of them changed --, and
// the Miller value / the exponentiation's value comes back as canonical bytes. Import and export are copies with a Montgomery conversion, one lane per item.
#define MBLS_SLOT_SF 97            // 12 Fp: the Miller value of (S, -G1) between the wave programs smiller and vmfinal (tools/gen_coop.py WS_G)
// item i's 13 values (apk X, Y, Z; sig x.c0 .. y.c1; H X.c0 .. Z.c1) -> slots APK 0..2, SIG 3..6 and h_slot .. h_slot + 5 (H, or S for program smiller)
__global__ void __launch_bounds__(WG) k_pair_import(mbls_ws ws, const uint8_t* in624, uint64_t n, int h_slot) {
    const uint64_t i = gid(); if (i >= n) return;
    for (int k = 0; k < 13; k++) ws_st(ws, k < MBLS_SLOT_H ? k : h_slot + (k - MBLS_SLOT_H), i, fp_to_mont(fp_raw_from_be(in624 + 624 * i + 48 * k)));
}
// item i's 12 coefficients -> slot F; one_slot >= 0: the element 1 into slots one_slot .. one_slot + 11 beside it
__global__ void __launch_bounds__(WG) k_f12_import(mbls_ws ws, const uint8_t* f576, uint64_t n, int one_slot) {
    const uint64_t i = gid(); if (i >= n) return;
    for (int k = 0; k < 12; k++) ws_st(ws, MBLS_SLOT_F + k, i, fp_to_mont(fp_raw_from_be(f576 + 576 * i + 48 * k)));
    if (one_slot >= 0) for (int k = 0; k < 12; k++) ws_st(ws, one_slot + k, i, k ? fp_zero() : fp_one());
}
__global__ void __launch_bounds__(WG) k_f12_export(mbls_ws ws, uint64_t n, int slot, uint8_t* out576) {
    const uint64_t i = gid(); if (i >= n) return;
    for (int k = 0; k < 12; k++) fp_raw_to_be(out576 + 576 * i + 48 * k, fp_from_mont(ws_ld(ws, slot + k, i)));
}
// the compiled two-pair loop (lane_miller without an LDS home for the running points: miller_loop of mbls_pairing.h)
__global__ void MBLS_LB k_miller_body(mbls_ws ws, uint64_t n) {
    uint64_t i = gid(); if (i >= n) return;
    lane_miller(ws, i);
}
// The final exponentiation with its VALUE kept: k_final / k_final2 with the fold into the status word replaced by a store of f (slot F of the item) and of
// fp12_is_one(&f) as the kernel evaluates it. The same launch bounds, the same LDS array, the same generated routines.
__global__ void MBLS_LB k_fexp_probe(mbls_ws ws, uint8_t* is_one, uint64_t n) {
#if MBLS_DEVICE_ASM
    __shared__ uint32_t accstore[154 * 64];
    uint64_t i = gid(); if (i >= n) return;
    fp12 f; final_exp_ws_d(&f, ws.w, ws.stride, i, (MBLS_LDS uint32_t*)accstore, threadIdx.x);
    is_one[i] = fp12_is_one(&f) ? 1 : 0;
    const fp2* c = &f.c0.c0;
#pragma unroll
    for (int s = 0; s < 6; s++) ws_st2(ws, MBLS_SLOT_F + 2 * s, i, c[s]);
#endif
}
// lanes 2 j, 2 j + 1 = item 32 blockIdx + j: the even lane stores value and bit, the odd lane compares its own words with the even lane's (its neighbour in the
// wave) and stores lanes_equal[i]
__global__ void MBLS_LB k_fexp2_probe(mbls_ws ws, uint8_t* is_one, uint8_t* lanes_equal, uint64_t n) {
#if MBLS_DEVICE_ASM
    __shared__ uint32_t accstore[154 * 64];
    const uint64_t t = gid(); if (t >= 2 * n) return;
    const uint64_t i = t >> 1;
    fp12 f; final_exp_ws_d2(&f, ws.w, ws.stride, i, (MBLS_LDS uint32_t*)accstore, threadIdx.x);
    const fp* c = &f.c0.c0.c0;
    uint32_t diff = 0;
#pragma unroll
    for (int k = 0; k < 12; k++) {
        const fp v = c[k];
#pragma unroll
        for (int j = 0; j < 12; j++) diff |= v[j] ^ (uint32_t)__shfl_xor((int)v[j], 1);
    }
    if (t & 1) { lanes_equal[i] = diff == 0 ? 1 : 0; return; }
    is_one[i] = fp12_is_one(&f) ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 12; k++) ws_st(ws, MBLS_SLOT_F + k, i, c[k]);
#endif
}
// the compiled body (lane_final's fallback: final_exp of mbls_pairing.h)
__global__ void MBLS_LB k_fexp_body(mbls_ws ws, uint8_t* is_one, uint64_t n) {
    uint64_t i = gid(); if (i >= n) return;
    fp12 f; fp2* c = &f.c0.c0;
    for (int s = 0; s < 6; s++) c[s] = ws_ld2(ws, MBLS_SLOT_F + 2 * s, i);
    final_exp(&f, &f);
    is_one[i] = fp12_is_one(&f) ? 1 : 0;
    for (int s = 0; s < 6; s++) ws_st2(ws, MBLS_SLOT_F + 2 * s, i, c[s]);
}
extern "C" int mbls_miller_probe(mbls_ctx* c, const uint8_t* in624, uint64_t n, uint8_t* out576, int mode) {
    if (!c || !out576 || (!in624 && n) || mode < 0 || mode > 5) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (!n) return MBLS_OK;
    if (!all_below_p(in624, 13 * n)) ARGFAIL(c, "a field element is not below p");
    HIPCHK(c, hipSetDevice(c->device));
    sbuf din(c, 0), dout(c, 1); HIPCHK(c, din.up(in624, 624 * n)); HIPCHK(c, dout.alloc(576 * n));
    int rc = mbls_ctx_reserve(c, n); if (rc) return rc;
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    hipStream_t s = c->hs_a;
    rc = ws_acquire(c, s); if (rc) return rc;
    hipLaunchKernelGGL(k_pair_import, dim3(nblk(n)), dim3(WG), 0, s, ws, din.as<uint8_t>(), n, mode == 5 ? MBLS_SLOT_S : MBLS_SLOT_H);
    if (mode == 0) hipLaunchKernelGGL(k_miller_body, dim3(nblk(n)), dim3(WG), 0, s, ws, n);
    else if (mode == 1) hipLaunchKernelGGL(k_miller, dim3(nblk(n)), dim3(WG), 0, s, ws, n);
    else if (mode == 2) hipLaunchKernelGGL(k_miller_single, dim3(nblk(n)), dim3(WG), 0, s, ws, n, 0, (uint64_t)0);
    else if (mode == 3) hipLaunchKernelGGL(k_miller_single2, dim3(nblk(2 * n)), dim3(WG), 0, s, ws, n, 0, (uint64_t)0);
    else coop_run(c, mode == 4 ? COOP_MILLER1 : COOP_SMILLER, ws, (uint64_t)0, (uint64_t)1, (uint64_t)0, n, (uint32_t*)nullptr, (uint8_t*)nullptr, COOP_RES_ITEM, s);
    hipLaunchKernelGGL(k_f12_export, dim3(nblk(n)), dim3(WG), 0, s, ws, n, mode == 5 ? MBLS_SLOT_SF : MBLS_SLOT_F, dout.as<uint8_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s)); c->ws_pending = false; HIPCHK(c, dout.down(out576, 576 * n)); return MBLS_OK;
}
extern "C" int mbls_final_exp_probe(mbls_ctx* c, const uint8_t* f576, uint64_t n, uint8_t* out576, uint8_t* is_one, int mode) {
    if (!c || !is_one || (!f576 && n) || mode < 0 || mode > 3 || (mode != 3 && !out576)) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (!n) return MBLS_OK;
    if (!all_below_p(f576, 12 * n)) ARGFAIL(c, "a field element is not below p");
    HIPCHK(c, hipSetDevice(c->device));
    sbuf din(c, 0), dout(c, 1), dbit(c, 2), deq(c, 3);
    HIPCHK(c, din.up(f576, 576 * n)); HIPCHK(c, dout.alloc(576 * n)); HIPCHK(c, dbit.alloc(n)); HIPCHK(c, deq.alloc(n));
    int rc = mbls_ctx_reserve(c, n); if (rc) return rc;
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    hipStream_t s = c->hs_a;
    rc = ws_acquire(c, s); if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(dbit.p, 0, n, s)); HIPCHK(c, hipMemsetAsync(deq.p, 0, n, s));
    hipLaunchKernelGGL(k_f12_import, dim3(nblk(n)), dim3(WG), 0, s, ws, din.as<uint8_t>(), n, mode == 3 ? MBLS_SLOT_SF : -1);
    if (mode == 0) hipLaunchKernelGGL(k_fexp_body, dim3(nblk(n)), dim3(WG), 0, s, ws, dbit.as<uint8_t>(), n);
    else if (mode == 1) hipLaunchKernelGGL(k_fexp_probe, dim3(nblk(n)), dim3(WG), 0, s, ws, dbit.as<uint8_t>(), n);
    else if (mode == 2) hipLaunchKernelGGL(k_fexp2_probe, dim3(nblk(2 * n)), dim3(WG), 0, s, ws, dbit.as<uint8_t>(), deq.as<uint8_t>(), n);
    else {            // program vmfinal on a wave per item: (slot F) * conj(1), the exponentiation, == 1 -- folded into a cleared status word, so results[item] is the bit
        HIPCHK(c, hipMemsetAsync(c->d_status, 0, 4 * n, s));
        coop_run(c, COOP_VMFINAL, ws, (uint64_t)0, (uint64_t)1, (uint64_t)0, n, c->d_status, dbit.as<uint8_t>(), COOP_RES_ITEM, s);
    }
    if (mode != 3) hipLaunchKernelGGL(k_f12_export, dim3(nblk(n)), dim3(WG), 0, s, ws, n, (int)MBLS_SLOT_F, dout.as<uint8_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s)); c->ws_pending = false;
    HIPCHK(c, dbit.down(is_one, n));
    if (mode != 3) HIPCHK(c, dout.down(out576, 576 * n));
    if (mode == 2) {                // bit 1: the odd lane of the item came back with the even lane's value
        std::vector<uint8_t> eq(n); HIPCHK(c, deq.down(eq.data(), n));
        for (uint64_t i = 0; i < n; i++) is_one[i] |= (uint8_t)(eq[i] << 1);
    }
    return MBLS_OK;
}
extern "C" int mbls_aggregate_public_keys_batch(mbls_ctx* c, const uint8_t* pks, int fmt, const uint32_t* off, uint64_t n, uint32_t k,
                                                uint8_t* apks96, uint32_t* status) {
    if (!c || !apks96 || (fmt != 0 && fmt != 1)) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (!n) return MBLS_OK;
    if (off && !offsets_ok(off, n)) ARGFAIL(c, "offsets must be non-decreasing");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = mbls_ctx_reserve(c, n); if (rc) return rc;
    uint64_t total = off ? off[n] : (uint64_t)k * n;
    if (total && !pks) ARGFAIL(c, "null key buffer");
    sbuf dp(c, 0), doff(c, 1), dout(c, 2); HIPCHK(c, dp.up(pks, (fmt ? 96 : 48) * total)); if (off) HIPCHK(c, doff.up(off, 4 * (n + 1))); HIPCHK(c, dout.alloc(96 * n));
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    hipStream_t s = c->hs_a;
    rc = ws_acquire(c, s); if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_status, 0, 4 * n, s));      // k_aggregate ORs its bits in
    launch_aggregate(ws, dp.as<uint8_t>(), off ? doff.as<uint32_t>() : (const uint32_t*)nullptr, k, fmt, MBLS_MODE_FAST_AGGREGATE, c->d_status, n, s);
    hipLaunchKernelGGL(k_apk_export, dim3(nblk(n)), dim3(WG), 0, s, ws, n, dout.as<uint8_t>());
    HIPCHK(c, hipStreamSynchronize(s)); c->ws_pending = false;
    HIPCHK(c, dout.down(apks96, 96 * n));
    if (status) HIPCHK(c, hipMemcpy(status, c->d_status, 4 * n, hipMemcpyDeviceToHost));
    return MBLS_OK;
}
extern "C" int mbls_aggregate_signatures_batch_device(mbls_ctx* c, const uint8_t* d_sigs, const uint32_t* d_off, uint64_t n, uint32_t k, uint64_t total,
                                                      uint8_t* d_out96, uint8_t* d_errs, void* stream) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (!n) return MBLS_OK;
    if (!d_out96 || !d_errs || (total && !d_sigs)) ARGFAIL(c, "null buffer");
    if (!d_off && total != (uint64_t)k * n) ARGFAIL(c, "total_sigs != n_sets * k");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    // the decoded points pass through two of the context's staging buffers: ordered against calls on other streams like the workspace
    // (a buffer that has to grow is freed, which drains the device first)
    int rc = ws_acquire(c, s); if (rc) return rc;
    sbuf dxy(c, 7), dfl(c, 8); HIPCHK(c, dxy.alloc(192 * total)); HIPCHK(c, dfl.alloc(total));
    if (total) hipLaunchKernelGGL(k_g2_decode_affine, dim3(nblk(total)), dim3(WG), 0, s, d_sigs, total, dxy.as<uint32_t>(), dfl.as<uint8_t>());
    hipLaunchKernelGGL(k_g2_sum, dim3(nblk(n)), dim3(WG), 0, s, (const uint32_t*)dxy.as<uint32_t>(), (const uint8_t*)dfl.as<uint8_t>(), d_off, k, n, d_out96, d_errs);
    HIPCHK(c, hipGetLastError());
    return ws_release(c, s);
}
extern "C" int mbls_aggregate_signatures_batch(mbls_ctx* c, const uint8_t* sigs, const uint32_t* off, uint64_t n, uint32_t k, uint8_t* out96, uint8_t* errs) {
    if (!c || !out96 || !errs) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (!n) return MBLS_OK;
    if (off && !offsets_ok(off, n)) ARGFAIL(c, "offsets must be non-decreasing");
    uint64_t total = off ? off[n] : (uint64_t)k * n;
    if (total && !sigs) ARGFAIL(c, "null signature buffer");
    HIPCHK(c, hipSetDevice(c->device));
    sbuf di(c, 0), doff(c, 1), dout(c, 2), de(c, 3);
    HIPCHK(c, di.up(sigs, 96 * total)); if (off) HIPCHK(c, doff.up(off, 4 * (n + 1))); HIPCHK(c, dout.alloc(96 * n)); HIPCHK(c, de.alloc(n));
    int rc = mbls_aggregate_signatures_batch_device(c, di.as<uint8_t>(), off ? doff.as<uint32_t>() : nullptr, n, k, total, dout.as<uint8_t>(), de.as<uint8_t>(), c->hs_a);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->hs_a)); HIPCHK(c, dout.down(out96, 96 * n)); HIPCHK(c, de.down(errs, n));
    for (uint64_t i = 0; i < n; i++) errs[i] = (uint8_t)map_dec_err_g2(errs[i]);
    return MBLS_OK;
}
extern "C" int mbls_fp_mul_batch(mbls_ctx* c, const uint8_t* a, const uint8_t* b, uint64_t n, uint8_t* out, int square) {
    if (!c || !a || !b || !out) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (!n) return MBLS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    sbuf da(c, 0), db(c, 1), dout(c, 2); HIPCHK(c, da.up(a, 48 * n)); HIPCHK(c, db.up(b, 48 * n)); HIPCHK(c, dout.alloc(48 * n));
    hipLaunchKernelGGL(k_fp_mul, dim3(nblk(n)), dim3(WG), 0, c->hs_a, da.as<uint8_t>(), db.as<uint8_t>(), n, dout.as<uint8_t>(), square);
    HIPCHK(c, hipStreamSynchronize(c->hs_a)); HIPCHK(c, dout.down(out, 48 * n)); return MBLS_OK;
}
#ifndef MBLS_DFORM_PROBE_NOPS
#include "mbls_towerd_asm.inc"          // the host pass does not see the generated routines: here only for the probes' shape tables (macros, no code)
#endif
static const uint32_t DFORM_PROBE_NIN[MBLS_DFORM_PROBE_NOPS] = MBLS_DFORM_PROBE_NIN, DFORM_PROBE_NOUT[MBLS_DFORM_PROBE_NOPS] = MBLS_DFORM_PROBE_NOUT;
extern "C" int mbls_dform_probe_shape(int op, uint32_t* n_in, uint32_t* n_out) {
    if (op < 0 || op >= MBLS_DFORM_PROBE_NOPS || !n_in || !n_out) return MBLS_ERR_ARGUMENT;
    *n_in = DFORM_PROBE_NIN[op]; *n_out = DFORM_PROBE_NOUT[op]; return MBLS_OK;
}
extern "C" int mbls_dform_probe(mbls_ctx* c, int op, const int32_t* in, uint64_t n, int32_t* out) {
    if (!c || !in || !out) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (op < 0 || op >= MBLS_DFORM_PROBE_NOPS) ARGFAIL(c, "no such probe");
    if (n > (1u << 24)) ARGFAIL(c, "at most 2^24 lanes per probe launch");
    if (!n) return MBLS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bin = (size_t)4 * DFORM_PROBE_NIN[op] * n, bout = (size_t)4 * DFORM_PROBE_NOUT[op] * n;
    sbuf di(c, 0), dout(c, 1), dran(c, 2); HIPCHK(c, di.up(in, bin)); HIPCHK(c, dout.alloc(bout));
    uint32_t ran = 0; HIPCHK(c, dran.up(&ran, 4));
    hipLaunchKernelGGL(k_dform_probe, dim3(nblk(n)), dim3(WG), 0, c->hs_a, di.as<int32_t>(), dout.as<int32_t>(), n, op, dran.as<uint32_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->hs_a)); HIPCHK(c, dran.down(&ran, 4));
    if (!ran) { snprintf(c->err, sizeof(c->err), "this build has no generated digit-form routines: nothing ran"); return MBLS_ERR_DEVICE; }
    HIPCHK(c, dout.down(out, bout)); return MBLS_OK;
}
// Test probe (include/mbls.h, "what the secret-key entries leave behind"): every device allocation the context owns, by name and size, and a copy of a byte
// range of one of them to the host once the device has drained. Reads only: no kernel, no secret. tests/test_secret_residue_cpu.py holds this table against the
// device pointers of struct mbls_ctx -- a new allocation goes here too (an allocation that does not exist yet is listed with 0 bytes, so the indices are stable).
struct residue_region { const char* name; const void* p; uint64_t bytes; };
#define RESIDUE_REGION(member, bytes) {#member, (const void*)c->member, (uint64_t)(c->member ? (bytes) : 0)}
#define MBLS_RESIDUE_REGIONS (20 + MBLS_N_STAGE)
static void residue_table(const mbls_ctx* c, residue_region* r) {
    const residue_region fixed[20] = {
        RESIDUE_REGION(d_w, (uint64_t)MBLS_SLOT_TOTAL * 12 * c->cap * 4),
        RESIDUE_REGION(d_status, c->cap * 4),
        RESIDUE_REGION(d_results, c->cap),
        RESIDUE_REGION(d_scalar, 64),
        RESIDUE_REGION(d_skidx, c->skidx_cap * 64 * 4),
        RESIDUE_REGION(d_sksel, c->sksel_cap * 64 * MBLS_KEYREC_DWORDS * 4),
        RESIDUE_REGION(d_keys_xy, c->key_cap * 96),
        RESIDUE_REGION(d_key_flags, c->key_cap),
        RESIDUE_REGION(d_htab, (uint64_t)MBLS_H_DWORDS * c->htab_cap * 4),
        RESIDUE_REGION(d_hflag, c->htab_cap * 4),
        RESIDUE_REGION(d_hst, c->htab_cap * 4),
        RESIDUE_REGION(d_hgrp, (uint64_t)MBLS_HGRP_ARRAYS * c->hgrp_cap * 4),
        RESIDUE_REGION(d_vmap, c->cap * 4),
        RESIDUE_REGION(d_cmt_list, c->cmt_words * 4),
        RESIDUE_REGION(d_cmt_cnt, c->cmt_items * 2 * 4),
        RESIDUE_REGION(d_cms_list, c->cms_words * 4),
        RESIDUE_REGION(d_cms_rec, c->cms_items * MBLS_CMS_REC_DWORDS * 4),
        RESIDUE_REGION(d_cms_park, c->cms_items * MBLS_CMS_PARK_DWORDS * 4),
        RESIDUE_REGION(d_coop, c->coop_bytes),
        RESIDUE_REGION(d_gtab, (uint64_t)1024 * MBLS_KEYREC_DWORDS * 4),
    };
    static const char* const stage_names[MBLS_N_STAGE] = {"stage[0]", "stage[1]", "stage[2]", "stage[3]", "stage[4]", "stage[5]", "stage[6]", "stage[7]", "stage[8]",
                                                          "stage[9]", "stage[10]"};
    for (int i = 0; i < 20; i++) r[i] = fixed[i];
    for (int i = 0; i < MBLS_N_STAGE; i++) r[20 + i] = residue_region{stage_names[i], c->stage[i].p, c->stage[i].p ? (uint64_t)c->stage[i].cap : 0};
}
extern "C" int mbls_ctx_residue_regions(mbls_ctx* c, char* names, uint64_t* bytes, uint32_t max_regions, uint32_t* n_regions, uint64_t* cap) {
    if (!c || !n_regions) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    *n_regions = MBLS_RESIDUE_REGIONS;
    if (cap) *cap = c->cap;
    if (!names && !bytes) return MBLS_OK;                // the count alone
    if (!names || !bytes || max_regions < MBLS_RESIDUE_REGIONS) ARGFAIL(c, "residue_regions: room for fewer regions than the context has");
    residue_region r[MBLS_RESIDUE_REGIONS]; residue_table(c, r);
    for (int i = 0; i < MBLS_RESIDUE_REGIONS; i++) {
        memset(names + MBLS_RESIDUE_NAME_BYTES * i, 0, MBLS_RESIDUE_NAME_BYTES); strncpy(names + MBLS_RESIDUE_NAME_BYTES * i, r[i].name, MBLS_RESIDUE_NAME_BYTES - 1);
        bytes[i] = r[i].bytes;
    }
    return MBLS_OK;
}
extern "C" int mbls_ctx_residue_read(mbls_ctx* c, uint32_t region, uint64_t offset, uint64_t bytes, uint8_t* out) {
    if (!c || (!out && bytes)) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (region >= MBLS_RESIDUE_REGIONS) ARGFAIL(c, "residue_read: no such region");
    residue_region r[MBLS_RESIDUE_REGIONS]; residue_table(c, r);
    if (offset > r[region].bytes || bytes > r[region].bytes - offset) ARGFAIL(c, "residue_read: the range leaves the region");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());                   // every stream of the context, and the caller's: what is read is what the calls so far left behind
    if (bytes) HIPCHK(c, hipMemcpy(out, (const uint8_t*)r[region].p + offset, bytes, hipMemcpyDeviceToHost));
    return MBLS_OK;
}
extern "C" int mbls_fp_mul_bench(mbls_ctx* c, uint64_t n_lanes, uint32_t iters, float* ms_out) {
    if (!c || !ms_out || !n_lanes) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    sbuf sink(c, 0); HIPCHK(c, sink.alloc(4 * n_lanes));
    hipLaunchKernelGGL(k_fp_mul_bench, dim3(nblk(n_lanes)), dim3(WG), 0, c->hs_a, sink.as<uint32_t>(), 16u, n_lanes);   // warm-up
    HIPCHK(c, hipEventRecord(c->ev[0], c->hs_a));
    hipLaunchKernelGGL(k_fp_mul_bench, dim3(nblk(n_lanes)), dim3(WG), 0, c->hs_a, sink.as<uint32_t>(), iters, n_lanes);
    HIPCHK(c, hipEventRecord(c->ev[1], c->hs_a)); HIPCHK(c, hipEventSynchronize(c->ev[1]));
    HIPCHK(c, hipEventElapsedTime(ms_out, c->ev[0], c->ev[1]));
    return MBLS_OK;
}

extern "C" int mbls_valu_bench(mbls_ctx* c, int mode, uint32_t waves_per_simd, uint32_t iters, float* ms_out) {
    if (!c || !ms_out || !waves_per_simd || waves_per_simd > 8 || mode < 0 || mode > 7) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    hipDeviceProp_t prop; HIPCHK(c, hipGetDeviceProperties(&prop, c->device));
    unsigned blocks = (unsigned)prop.multiProcessorCount * 4u * waves_per_simd;      // waves_per_simd waves on every SIMD
    sbuf sink(c, 0); HIPCHK(c, sink.alloc((size_t)4 * WG * blocks));
    hipLaunchKernelGGL(k_valu_bench, dim3(blocks), dim3(WG), 0, c->hs_a, sink.as<uint32_t>(), 64u, mode);     // warm-up
    HIPCHK(c, hipEventRecord(c->ev[0], c->hs_a));
    hipLaunchKernelGGL(k_valu_bench, dim3(blocks), dim3(WG), 0, c->hs_a, sink.as<uint32_t>(), iters, mode);
    HIPCHK(c, hipEventRecord(c->ev[1], c->hs_a)); HIPCHK(c, hipEventSynchronize(c->ev[1]));
    HIPCHK(c, hipEventElapsedTime(ms_out, c->ev[0], c->ev[1]));
    return MBLS_OK;
}

// ---- scalar API (n = 1 batches)
static int sk_check(const uint8_t* sk, size_t len) {     // SecretKey::from_bytes, reference src/keys.rs:80-82 and tests :285-297
    static const uint8_t R_BE[32] = {0x73,0xed,0xa7,0x53,0x29,0x9d,0x7d,0x48,0x33,0x39,0xd8,0x08,0x09,0xa1,0xd8,0x05,0x53,0xbd,0xa4,0x02,0xff,0xfe,0x5b,0xfe,0xff,0xff,0xff,0xff,0x00,0x00,0x00,0x01};
    if (!sk || len != 32) return MBLS_ERR_INVALID_SECRET_KEY_SIZE;
    bool zero = true; for (int i = 0; i < 32; i++) if (sk[i]) zero = false;
    if (zero || memcmp(sk, R_BE, 32) >= 0) return MBLS_ERR_INVALID_SECRET_KEY_RANGE;
    return MBLS_OK;
}
extern "C" int mbls_pk_from_bytes(mbls_ctx* c, const uint8_t* bytes, size_t len, uint8_t pk_out[96]) {
    if (!c || !pk_out) return MBLS_ERR_ARGUMENT;
    if (!bytes || len != 48) return MBLS_ERR_INVALID_G1_SIZE;         // decompress_g1, reference src/amcl_utils.rs:54-56
    uint8_t e; int rc = mbls_pk_decode_batch(c, bytes, MBLS_PK_COMPRESSED, 1, 1, pk_out, &e); return rc ? rc : e;
}
extern "C" int mbls_pk_from_bytes_unchecked(mbls_ctx* c, const uint8_t* bytes, size_t len, uint8_t pk_out[96]) {
    if (!c || !pk_out) return MBLS_ERR_ARGUMENT;
    if (!bytes || len != 48) return MBLS_ERR_INVALID_G1_SIZE;
    uint8_t e; int rc = mbls_pk_decode_batch(c, bytes, MBLS_PK_COMPRESSED, 0, 1, pk_out, &e); return rc ? rc : e;
}
extern "C" int mbls_pk_from_uncompressed_bytes(mbls_ctx* c, const uint8_t* bytes, size_t len, uint8_t pk_out[96]) {
    if (!c || !pk_out) return MBLS_ERR_ARGUMENT;
    if (!bytes || len != 96) return MBLS_ERR_INVALID_G1_SIZE;         // reference src/keys.rs:171-173
    uint8_t e; int rc = mbls_pk_decode_batch(c, bytes, MBLS_PK_UNCOMPRESSED, 0, 1, pk_out, &e); return rc ? rc : e;
}
extern "C" int mbls_pk_as_bytes(mbls_ctx* c, const uint8_t pk[96], uint8_t out[48]) {
    if (!c || !pk || !out) return MBLS_ERR_ARGUMENT;
    uint8_t e; int rc = mbls_pk_compress_batch(c, pk, 1, out, &e); return rc ? rc : e;
}
extern "C" int mbls_pk_key_validate(mbls_ctx* c, const uint8_t pk[96]) {
    if (!c || !pk) return 0;
    mbls_lock lk(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return 0;
    sbuf di(c, 0), dk(c, 1); if (di.up(pk, 96) != hipSuccess || dk.alloc(1) != hipSuccess) return 0;
    hipLaunchKernelGGL(k_g1_key_validate, dim3(1), dim3(WG), 0, c->hs_a, di.as<uint8_t>(), (uint64_t)1, dk.as<uint8_t>());
    uint8_t ok = 0; if (hipStreamSynchronize(c->hs_a) != hipSuccess || dk.down(&ok, 1) != hipSuccess) return 0;
    return ok;
}
extern "C" int mbls_pk_from_secret_key(mbls_ctx* c, const uint8_t* sk, size_t sk_len, uint8_t pk_out[96]) {
    if (!c || !pk_out) return MBLS_ERR_ARGUMENT;
    int e = sk_check(sk, sk_len); if (e) return e;
    return mbls_sk_to_pk_batch(c, sk, MBLS_PK_UNCOMPRESSED, 1, pk_out);
}
extern "C" int mbls_sig_from_bytes(mbls_ctx* c, const uint8_t* bytes, size_t len, uint8_t sig_out[96]) {
    if (!c || !sig_out) return MBLS_ERR_ARGUMENT;
    if (!bytes || len != 96) return MBLS_ERR_INVALID_G2_SIZE;         // decompress_g2, reference src/amcl_utils.rs:70-72
    uint8_t e; int rc = mbls_sig_check_batch(c, bytes, 1, &e, nullptr); if (rc) return rc;
    if (e) return e;
    memcpy(sig_out, bytes, 96); return MBLS_OK;
}
extern "C" int mbls_sign(mbls_ctx* c, const uint8_t* msg, size_t msg_len, const uint8_t* sk, size_t sk_len, uint8_t sig_out[96]) {
    if (!c || !sig_out) return MBLS_ERR_ARGUMENT;
    if (msg_len > 0xFFFFFFFFull) return MBLS_ERR_ARGUMENT;
    int e = sk_check(sk, sk_len); if (e) return e;
    return mbls_sign_batch(c, sk, msg, (uint32_t)msg_len, 1, sig_out);
}
extern "C" int mbls_verify(mbls_ctx* c, const uint8_t sig[96], const uint8_t* msg, size_t msg_len, const uint8_t pk[96]) {
    uint8_t r = 0; if (!c || !sig || !pk || msg_len > 0xFFFFFFFFull) return 0;
    if (mbls_verify_batch(c, sig, msg, (uint32_t)msg_len, nullptr, pk, MBLS_PK_UNCOMPRESSED, 1, &r, nullptr)) return 0;
    return r;
}
extern "C" int mbls_aggregate_public_keys(mbls_ctx* c, const uint8_t* pks96, size_t n, uint8_t apk_out[96]) {
    if (!c || !apk_out) return MBLS_ERR_ARGUMENT;
    if (n == 0) return MBLS_ERR_AGGREGATE_EMPTY_POINTS;               // reference src/aggregates.rs:30-32
    if (n > 0xFFFFFFFFull) return MBLS_ERR_ARGUMENT;
    uint32_t st = 0; int rc = mbls_aggregate_public_keys_batch(c, pks96, MBLS_PK_UNCOMPRESSED, nullptr, 1, (uint32_t)n, apk_out, &st);
    if (rc) return rc;
    return (st & MBLS_ST_BAD_PK_ENCODING) ? MBLS_ERR_INVALID_POINT : MBLS_OK;
}
extern "C" int mbls_aggregate_public_key_add(mbls_ctx* c, const uint8_t a[96], const uint8_t b[96], uint8_t out[96]) {
    if (!c || !a || !b || !out) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    sbuf da(c, 0), db(c, 1), dout(c, 2), de(c, 3); HIPCHK(c, da.up(a, 96)); HIPCHK(c, db.up(b, 96)); HIPCHK(c, dout.alloc(96)); HIPCHK(c, de.alloc(1));
    hipLaunchKernelGGL(k_g1_add, dim3(1), dim3(WG), 0, c->hs_a, da.as<uint8_t>(), db.as<uint8_t>(), (uint64_t)1, dout.as<uint8_t>(), de.as<uint8_t>());
    uint8_t e; HIPCHK(c, hipStreamSynchronize(c->hs_a)); HIPCHK(c, dout.down(out, 96)); HIPCHK(c, de.down(&e, 1));
    return map_dec_err_g1(e);
}
extern "C" int mbls_aggregate_signature_add(mbls_ctx* c, const uint8_t a[96], const uint8_t b[96], uint8_t out[96]) {
    if (!c || !a || !b || !out) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    sbuf da(c, 0), db(c, 1), dout(c, 2), de(c, 3); HIPCHK(c, da.up(a, 96)); HIPCHK(c, db.up(b, 96)); HIPCHK(c, dout.alloc(96)); HIPCHK(c, de.alloc(1));
    hipLaunchKernelGGL(k_g2_add, dim3(1), dim3(WG), 0, c->hs_a, da.as<uint8_t>(), db.as<uint8_t>(), (uint64_t)1, dout.as<uint8_t>(), de.as<uint8_t>());
    uint8_t e; HIPCHK(c, hipStreamSynchronize(c->hs_a)); HIPCHK(c, dout.down(out, 96)); HIPCHK(c, de.down(&e, 1));
    return map_dec_err_g2(e);
}
extern "C" int mbls_fast_aggregate_verify(mbls_ctx* c, const uint8_t sig[96], const uint8_t* msg, size_t msg_len, const uint8_t* pks96, size_t n_pks) {
    uint8_t r = 0; if (!c || !sig || msg_len > 0xFFFFFFFFull || n_pks > 0xFFFFFFFFull) return 0;
    if (n_pks == 0) return 0;                                         // reference src/aggregates.rs:179-181
    if (mbls_fast_aggregate_verify_batch(c, sig, msg, (uint32_t)msg_len, nullptr, pks96, MBLS_PK_UNCOMPRESSED, nullptr, 1, (uint32_t)n_pks, &r, nullptr)) return 0;
    return r;
}
extern "C" int mbls_fast_aggregate_verify_pre_aggregated(mbls_ctx* c, const uint8_t sig[96], const uint8_t* msg, size_t msg_len, const uint8_t apk[96]) {
    uint8_t r = 0; if (!c || !sig || !apk || msg_len > 0xFFFFFFFFull) return 0;
    // identical checks with a one-key set: sig in G2, key != infinity, pairing (reference src/aggregates.rs:223-253)
    if (mbls_fast_aggregate_verify_batch(c, sig, msg, (uint32_t)msg_len, nullptr, apk, MBLS_PK_UNCOMPRESSED, nullptr, 1, 1, &r, nullptr)) return 0;
    return r;
}

// Product / sum trees of the n-pairing paths: m values in slot F (slot S) of items 0..m-1 -> item 0. A level with many pairs is one lane
// per product (k_f12_tree_d / k_g2_tree_d: the chip is full of them); below MBLS_COOP_TREE_PAIRS pairs a level is one WAVE per product
// (mbls_coop.h, programs f12mul / g2add: 14 / 28 steps instead of a 25 k-instruction dependent chain).
#define MBLS_COOP_TREE_PAIRS 2048
static void f12_tree(mbls_ctx* c, mbls_ws ws, uint64_t m, hipStream_t s) {
    while (m > 1) {
        const uint64_t half = (m + 1) / 2, pairs = m - half;
        if (pairs > MBLS_COOP_TREE_PAIRS) hipLaunchKernelGGL(k_f12_tree_d, dim3(nblk(half)), dim3(WG), 0, s, ws, m, half);
        else coop_run(c, COOP_F12MUL, ws, (uint64_t)0, (uint64_t)1, half, pairs, (uint32_t*)nullptr, (uint8_t*)nullptr, COOP_RES_ITEM, s);
        m = half;
    }
}
static void g2_tree_levels(mbls_ctx* c, mbls_ws ws, uint64_t m, int levels, hipStream_t s) {
    while (m > 1 && levels-- > 0) {
        const uint64_t half = (m + 1) / 2, pairs = m - half;
        if (pairs > MBLS_COOP_TREE_PAIRS) hipLaunchKernelGGL(k_g2_tree_d, dim3(nblk(half)), dim3(WG), 0, s, ws, m, half);
        else coop_run(c, COOP_G2ADD, ws, (uint64_t)0, (uint64_t)1, half, pairs, (uint32_t*)nullptr, (uint8_t*)nullptr, COOP_RES_ITEM, s);
        m = half;
    }
}
static void g2_tree(mbls_ctx* c, mbls_ws ws, uint64_t m, hipStream_t s) { g2_tree_levels(c, ws, m, 64, s); }
// n-pairing product check shared by aggregate_verify and verify_multiple (reference src/aggregates.rs:158-169, :307-315). On entry the
// workspace holds, for items 0..n-1, H_i (slot H) and P_i (slot APK); S (the (S, -G1) pair's G2 point) in slot S of item 0; the OR of
// every status word in d_scalar[0]. Everything is enqueued on s: one Miller loop per lane, the product tree, and ONE wave for the tail --
// the Miller loop of (S, -G1), the product, the single final exponentiation, the comparison and the status bits (program vmtail).
// late_status: fold the sets' status words into d_scalar[0] only HERE, after the wait for the signature chain -- the sets' Miller loops then start as
// soon as the keys and the messages are ready and do not wait for the (longer) signature chain, whose bits only the tail needs
// d_partial: stop before the tail and write the shard's record instead (k_vm_export); s_miller_ev then only says "the signature chain is done"
// side_s_chain (batches that fill the chip and run their chains one after the other): the signatures' sum tree and the Miller loop of (S, -G1) are
// enqueued HERE on a second stream, beside the product tree -- both trees are short kernels on a shrinking number of lanes, and the one-wave
// Miller loop hides behind them
// m one-pair Miller loops over items [0, m) of ws (k_miller_single's layout), one lane per pair; half a round or less: two lanes per pair, products in
// pairs (4.9 ms instead of 6.7). Above a round the whole rounds go first and what is left of the last one follows as a launch of its own in the form
// its size allows (81 920 pairs: 6.7 + 4.9 ms instead of two rounds)
// d_live (calls over a resident message table): the device-side count of items that have a pair; the same cuts on k_vmt_miller / k_vmt_miller2
static void launch_miller_single(mbls_ctx* c, mbls_ws ws, uint64_t m, hipStream_t s, const uint32_t* d_live = nullptr) {
    const uint64_t R = c->round_items;
    const uint64_t full = m > R ? (m / R) * R : 0, rest = m - full;
    if (d_live) {
        if (full) hipLaunchKernelGGL(k_vmt_miller, dim3(nblk(full)), dim3(WG), 0, s, ws, full, (uint64_t)0, d_live);
        if (!rest) return;
        mbls_ws wr = ws; wr.w += full;
        if (2 * rest <= R) hipLaunchKernelGGL(k_vmt_miller2, dim3(nblk(2 * rest)), dim3(WG), 0, s, wr, rest, full, d_live);
        else hipLaunchKernelGGL(k_vmt_miller, dim3(nblk(rest)), dim3(WG), 0, s, wr, rest, full, d_live);
        return;
    }
    if (full) hipLaunchKernelGGL(k_miller_single, dim3(nblk(full)), dim3(WG), 0, s, ws, full, 0, (uint64_t)0);
    if (!rest) return;
    mbls_ws wr = ws; wr.w += full;
    if (2 * rest <= R) hipLaunchKernelGGL(k_miller_single2, dim3(nblk(2 * rest)), dim3(WG), 0, s, wr, rest, 0, (uint64_t)0);
    else hipLaunchKernelGGL(k_miller_single, dim3(nblk(rest)), dim3(WG), 0, s, wr, rest, 0, (uint64_t)0);
}
static int npairing_finish(mbls_ctx* c, uint64_t n, hipStream_t s, uint8_t* d_result, hipEvent_t s_miller_ev = nullptr, bool late_status = false,
                           uint32_t* d_partial = nullptr, bool side_s_chain = false, uint64_t n_sets = 0, uint64_t keep_f_at = 0, const uint32_t* d_live = nullptr) {
    // d_live (calls over a resident message table, grouped): the device-side count of Miller items that have a pair; waves without one return at once
    // n_sets (grouped shared-message route): the n Miller items are the MESSAGES; the signatures' sum tree and the status fold still cover all n_sets sets
    // keep_f_at (locate calls on the per-set route): the first shadow item -- the sets' Miller values are copied there before the product tree runs over them
    const uint64_t ns = n_sets ? n_sets : n;
    const bool s_miller_done = s_miller_ev != nullptr || side_s_chain;
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    if (2 * n <= c->coop_max_items)     // few pairs: one WAVE per Miller loop (program miller1, ~0.9 ms) instead of one lane (6.6 ms)
        coop_run(c, COOP_MILLER1, ws, (uint64_t)0, (uint64_t)1, (uint64_t)0, n, (uint32_t*)nullptr, (uint8_t*)nullptr, COOP_RES_ITEM, s, d_live);
    else
        launch_miller_single(c, ws, n, s, d_live);
    if (keep_f_at) hipLaunchKernelGGL(k_vml_keep_f, dim3(nblk(n)), dim3(WG), 0, s, ws, n, keep_f_at);
    if (side_s_chain) {
        HIPCHK(c, hipEventRecord(c->hs_ev2, s)); HIPCHK(c, hipStreamWaitEvent(c->hs_b, c->hs_ev2, 0));
        g2_tree(c, ws, ns, c->hs_b);
        if (!d_partial) coop_run(c, COOP_SMILLER, ws, (uint64_t)0, (uint64_t)1, (uint64_t)0, (uint64_t)1, (uint32_t*)nullptr, (uint8_t*)nullptr, COOP_RES_ITEM, c->hs_b);
        HIPCHK(c, hipEventRecord(c->hs_ev, c->hs_b));
        s_miller_ev = c->hs_ev;
    }
    f12_tree(c, ws, n, s);
    // s_miller_done: the Miller value of (S, -G1) is left in slots 97..108 of item 0 by program smiller, running beside the chains
    if (s_miller_done) HIPCHK(c, hipStreamWaitEvent(s, s_miller_ev, 0));
    if (late_status) hipLaunchKernelGGL(k_status_or, dim3(nblk(ns)), dim3(WG), 0, s, c->d_status, ns, c->d_scalar);
    if (d_partial) hipLaunchKernelGGL(k_vm_export, dim3(1), dim3(WG), 0, s, ws, (const uint32_t*)c->d_scalar, 0, d_partial);
    else coop_run(c, s_miller_done ? COOP_VMFINAL : COOP_VMTAIL, ws, (uint64_t)0, (uint64_t)1, (uint64_t)0, (uint64_t)1, c->d_scalar, d_result, COOP_RES_BATCH, s);
    HIPCHK(c, hipGetLastError());
    return MBLS_OK;
}
// Phase two of mbls_verify_multiple*_shared_msgs_locate* behind the mark kernel: the candidates' verdicts (cand[i]: set i is examined; st_set[i]: its own word).
// The Miller loops walk the m shadow items from item sh on in ONE launch, cut at rounds and put on lane pairs exactly as launch_miller_single decides for m
// items; then item i of the view wp takes the product with its partner i + half (a tree level), and a final exponentiation per candidate reads it.
//   per-set route: m = n shadows ([r_i] sig_i, -G1); wp = the workspace, half = sh: f_i (moved back to item i by k_vml_mark) times g_i
//   grouped route: m = 2 n shadows, A(i) = sh + i: (H(m_i), [r_i] apk_i), B(i) = sh + n + i: ([r_i] sig_i, -G1); wp = the view from A(0), half = n
static void vsl_examine(mbls_ctx* c, mbls_ws ws, uint64_t n, uint64_t sh, bool grouped, const uint32_t* st_set, const uint32_t* cand, uint8_t* d_set_results,
                        uint32_t* d_set_status, hipStream_t s) {
    const uint64_t R = c->round_items, m = grouped ? 2 * n : n;
    const uint64_t full = m > R ? (m / R) * R : 0, rest = m - full;
    mbls_ws wsh = ws; wsh.w += sh;
    if (full) hipLaunchKernelGGL(k_vsl_miller, dim3(nblk(full)), dim3(WG), 0, s, wsh, full, (uint64_t)0, n, cand);
    if (rest) {
        mbls_ws wr = wsh; wr.w += full;
        if (2 * rest <= R) hipLaunchKernelGGL(k_vsl_miller2, dim3(nblk(2 * rest)), dim3(WG), 0, s, wr, rest, full, n, cand);
        else hipLaunchKernelGGL(k_vsl_miller, dim3(nblk(rest)), dim3(WG), 0, s, wr, rest, full, n, cand);
    }
    const mbls_ws wp = grouped ? wsh : ws;
    hipLaunchKernelGGL(k_vml_product, dim3(nblk(n)), dim3(WG), 0, s, wp, n, grouped ? n : sh, cand);
    if (n <= c->split_max_items && 2 * n <= c->round_items)
        hipLaunchKernelGGL(k_vml_final2, dim3(nblk(2 * n)), dim3(WG), 0, s, wp, st_set, cand, d_set_results, d_set_status, n);
    else
        hipLaunchKernelGGL(k_vml_final, dim3(nblk(n)), dim3(WG), 0, s, wp, st_set, cand, d_set_results, d_set_status, n);
}
extern "C" int mbls_aggregate_verify(mbls_ctx* c, const uint8_t sig[96], const uint8_t* msgs, const size_t* msg_lens, size_t n_msgs,
                                     const uint8_t* pks96, size_t n_pks) {
    if (!c || !sig) return 0;
    if (n_msgs != n_pks || n_pks == 0) return 0;                      // reference src/aggregates.rs:132-134
    if (!msg_lens || !pks96) return 0;
    mbls_lock lk(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return 0;
    uint64_t n = n_pks;
    if (mbls_ctx_reserve(c, n)) return 0;
    std::vector<uint64_t> off;
    try { off.resize(n + 1); } catch (...) { return 0; }
    size_t total = 0;
    for (size_t i = 0; i < n; i++) {
        if (msg_lens[i] > 0xFFFFFFFFull) return 0;
        off[i] = total; total += msg_lens[i];
    }
    off[n] = total;
    if (total && !msgs) return 0;
    sbuf dm(c, 0), doff(c, 1), dp(c, 3), dsig(c, 4); int result = 0;
    if (dm.up(msgs, total) != hipSuccess || doff.up(off.data(), 8 * (n + 1)) != hipSuccess ||
        dp.up(pks96, 96 * n) != hipSuccess || dsig.up(sig, 96) != hipSuccess) return 0;
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    hipStream_t s = c->hs_a;
    if (ws_acquire(c, s)) return 0;
    (void)hipMemsetAsync(c->d_scalar, 0, 64, s);
    (void)hipMemsetAsync(c->d_status, 0, 4 * n, s);
    if (hipMemsetAsync(c->d_results, 0, 1, s) != hipSuccess) return 0;      // false until the tail kernel has spoken
    // three chains side by side: the signature (decode + subgroup test: k_sig on item 0's slots, then into slot S), the keys, the messages
    (void)hipEventRecord(c->hs_ev, s); (void)hipStreamWaitEvent(c->hs_b, c->hs_ev, 0); (void)hipStreamWaitEvent(c->hs_c, c->hs_ev, 0);
    hipLaunchKernelGGL(k_sig2, dim3(1), dim3(WG), 0, c->hs_b, ws, (const uint8_t*)dsig.as<uint8_t>(), c->d_status, (uint64_t)1);      // (two lanes: the chain is latency)
    hipLaunchKernelGGL(k_sigslot_to_s, dim3(1), dim3(WG), 0, c->hs_b, ws, (uint64_t)0);
    (void)hipEventRecord(c->hs_ev2, c->hs_b);                                   // the signature's status bits and S exist
    // ... and its Miller loop (S, -G1) runs on one wave right away, beside the message phase (the longest chain) and the pairs' own loops: the tail then only
    // multiplies and exponentiates (program vmfinal instead of vmtail)
    coop_run(c, COOP_SMILLER, ws, (uint64_t)0, (uint64_t)1, (uint64_t)0, (uint64_t)1, (uint32_t*)nullptr, (uint8_t*)nullptr, COOP_RES_ITEM, c->hs_b);
    (void)hipEventRecord(c->hs_ev, c->hs_b);
    hipLaunchKernelGGL(k_blind_g1, dim3(nblk(n)), dim3(WG), 0, s, ws, dp.as<uint8_t>(), (const uint64_t*)nullptr, c->d_status, n);   // r_i = 1: no blinding in AggregateVerify
    launch_hash(c, ws, dm.as<uint8_t>(), 0u, (const uint64_t*)doff.as<uint64_t>(), c->d_status, n, c->hs_c);
    (void)hipEventRecord(c->hs_ev3, c->hs_c);
    (void)hipStreamWaitEvent(s, c->hs_ev2, 0); (void)hipStreamWaitEvent(s, c->hs_ev3, 0);
    hipLaunchKernelGGL(k_status_or, dim3(nblk(n)), dim3(WG), 0, s, c->d_status, n, c->d_scalar);
    // a signature outside G2 or an undecodable member makes the tail answer false (reference src/aggregates.rs:137-139): no host round trip
    if (npairing_finish(c, n, s, c->d_results, c->hs_ev)) return 0;
    uint8_t r = 0;
    if (hipStreamSynchronize(s) != hipSuccess) return 0;
    c->ws_pending = false;
    if (hipMemcpy(&r, c->d_results, 1, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    result = r;
    return result;
}
// n x AggregateSignature::aggregate_verify (reference src/aggregates.rs:130-170): item i = (sig_i, its (message, key) pairs). The pairs of
// all items lie back to back: pair j = (message j of d_msgs / d_moff, key d_pks96 + 96 j); item i owns pairs [d_pair_off[i], d_pair_off[i+1])
// or k each. One lane per pair for the key, the message phase and the one-pair Miller loop; the (sig_i, -G1) pairs ride the same Miller
// launch; a product tree per item; one final exponentiation per item. Enqueues only.
extern "C" int mbls_aggregate_verify_batch_device(mbls_ctx* c, const uint8_t* d_sigs, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff,
        const uint8_t* d_pks96, const uint32_t* d_pair_off, uint32_t k, uint64_t total, uint64_t n, uint8_t* d_results, uint32_t* d_status, void* stream) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (n == 0) return MBLS_OK;
    if (!d_sigs || !d_results || (total && (!d_pks96 || (!d_msgs && msg_len && !d_moff)))) ARGFAIL(c, "null buffer");
    if (!d_pair_off && total != (uint64_t)k * n) ARGFAIL(c, "total_pairs != n * k");
    if (total > 0xFFFFFFFFull) ARGFAIL(c, "pair indices are 32-bit");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const uint64_t M = 2 * n + total;
    int rc = mbls_ctx_reserve(c, M); if (rc) return rc;
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    mbls_ws wp = ws; wp.w += n;                                   // the pairs' view: item j of wp = workspace item n + j
    rc = ws_acquire(c, s); if (rc) return rc;
    uint32_t* st_item = d_status ? d_status : c->d_status;
    uint32_t* st_pair = c->d_status + n;                         // (cap >= 2 n + T words)
    uint32_t* map = nullptr;
    sbuf dmap(c, 9);
    if (d_pair_off) {      // the staging buffer is reused between calls: every entry the map kernel does not write must read as "no owner"
        HIPCHK(c, dmap.alloc(4 * (total ? total : 1))); map = dmap.as<uint32_t>();
        HIPCHK(c, hipMemsetAsync(map, 0xFF, 4 * (total ? total : 1), s));
    }
    HIPCHK(c, hipMemsetAsync(st_item, 0, 4 * n, s));
    if (st_item != c->d_status) HIPCHK(c, hipMemsetAsync(c->d_status, 0, 4 * n, s));
    if (total) HIPCHK(c, hipMemsetAsync(st_pair, 0, 4 * total, s));
    HIPCHK(c, hipMemsetAsync(d_results, 0, n, s));                // false until k_final has spoken
    // three chains side by side while they leave SIMDs idle: signatures (items [0, n)), keys and messages (items [n, n + T) through wp)
    const bool fork = n + 2 * total <= c->fork_max_items;
    hipStream_t s_sig = fork ? c->hs_b : s, s_msg = fork ? c->hs_c : s;
    if (fork) { HIPCHK(c, hipEventRecord(c->hs_ev, s)); HIPCHK(c, hipStreamWaitEvent(s_sig, c->hs_ev, 0)); HIPCHK(c, hipStreamWaitEvent(s_msg, c->hs_ev, 0)); }
    hipLaunchKernelGGL(k_sig, dim3(nblk(n)), dim3(WG), 0, s_sig, ws, d_sigs, st_item, n, 1);
    hipLaunchKernelGGL(k_sigpair_setup, dim3(nblk(n)), dim3(WG), 0, s_sig, ws, n);
    if (total) {
        if (d_pair_off) hipLaunchKernelGGL(k_pair_item_map, dim3(nblk(n)), dim3(WG), 0, s, d_pair_off, n, total, map);
        hipLaunchKernelGGL(k_blind_g1, dim3(nblk(total)), dim3(WG), 0, s, wp, d_pks96, (const uint64_t*)nullptr, st_pair, total);      // decode only: r_i = 1
        launch_hash(c, wp, d_msgs, msg_len, d_moff, st_pair, total, s_msg);
    }
    if (fork) {
        HIPCHK(c, hipEventRecord(c->hs_ev2, s_sig)); HIPCHK(c, hipEventRecord(c->hs_ev3, s_msg));
        HIPCHK(c, hipStreamWaitEvent(s, c->hs_ev2, 0)); HIPCHK(c, hipStreamWaitEvent(s, c->hs_ev3, 0));
    }
    // one Miller loop per pair, the signatures' pairs included: items [0, n + T)
    if (2 * (n + total) <= c->coop_max_items)
        coop_run(c, COOP_MILLER1, ws, (uint64_t)0, (uint64_t)1, (uint64_t)0, n + total, (uint32_t*)nullptr, (uint8_t*)nullptr, COOP_RES_ITEM, s);
    else
        launch_miller_single(c, ws, n + total, s);
    // per-item product trees over the pairs, then item i <- (sig pair) x (its pairs' product)
    uint64_t kmax = d_pair_off ? total : k;                      // a ragged layout may hold one long range: levels up to the whole list
    for (uint64_t half = 1; half < kmax; half *= 2)
        hipLaunchKernelGGL(k_f12_seg_tree_d, dim3(nblk(total)), dim3(WG), 0, s, wp, (const uint32_t*)map, d_pair_off, k, n, total, half);
    hipLaunchKernelGGL(k_f12_seg_gather, dim3(nblk(n)), dim3(WG), 0, s, ws, d_pair_off, (const uint32_t*)map, k, n, total, st_item, (const uint32_t*)st_pair);
    hipLaunchKernelGGL(k_f12_tree_d, dim3(nblk(n)), dim3(WG), 0, s, ws, 2 * n + total, n + total);
    if (n <= c->split_max_items && 2 * n <= c->round_items) hipLaunchKernelGGL(k_final2, dim3(nblk(2 * n)), dim3(WG), 0, s, ws, st_item, d_results, n);
    else hipLaunchKernelGGL(k_final, dim3(nblk(n)), dim3(WG), 0, s, ws, st_item, d_results, n);
    HIPCHK(c, hipGetLastError());
    return ws_release(c, s);
}
extern "C" int mbls_aggregate_verify_batch(mbls_ctx* c, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len, const uint64_t* moff,
        const uint8_t* pks96, const uint32_t* pair_off, uint32_t k, uint64_t n, uint8_t* results, uint32_t* status) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (n == 0) return MBLS_OK;
    if (!sigs || !results) ARGFAIL(c, "null buffer");
    if (pair_off && (!offsets_ok(pair_off, n) || pair_off[0] != 0)) ARGFAIL(c, "pair_offsets must start at 0 and be non-decreasing");
    const uint64_t total = pair_off ? pair_off[n] : (uint64_t)k * n;
    if (moff && !msg_offsets_ok(moff, total)) ARGFAIL(c, "msg_offsets must be non-decreasing, messages below 2^32 bytes");
    const uint64_t msg_first = moff ? moff[0] : 0;
    const size_t msg_total = moff ? (size_t)(moff[total] - moff[0]) : (size_t)msg_len * total;
    if (total && (!pks96 || (!msgs && msg_total))) ARGFAIL(c, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    sbuf ds(c, 0), dm(c, 1), dp(c, 2), doff(c, 3), dr(c, 4), dst(c, 5), dmo(c, 6);
    HIPCHK(c, ds.up(sigs, 96 * n)); HIPCHK(c, dm.up(msgs ? msgs + msg_first : nullptr, msg_total)); HIPCHK(c, dp.up(pks96, 96 * total));
    if (pair_off) HIPCHK(c, doff.up(pair_off, 4 * (n + 1)));
    const uint8_t* d_msgs = dm.as<uint8_t>();
    if (moff) { HIPCHK(c, dmo.up(moff, 8 * (total + 1))); d_msgs -= msg_first; }
    HIPCHK(c, dr.alloc(n)); HIPCHK(c, dst.alloc(4 * n));
    int rc = mbls_aggregate_verify_batch_device(c, ds.as<uint8_t>(), d_msgs, msg_len, moff ? dmo.as<uint64_t>() : nullptr, dp.as<uint8_t>(),
                                                pair_off ? doff.as<uint32_t>() : nullptr, k, total, n, dr.as<uint8_t>(), dst.as<uint32_t>(), c->hs_a);
    if (rc) { (void)hipStreamSynchronize(c->hs_a); (void)hipStreamSynchronize(c->hs_b); (void)hipStreamSynchronize(c->hs_c); c->ws_pending = false; return rc; }
    HIPCHK(c, hipStreamSynchronize(c->hs_a));
    c->ws_pending = false;
    HIPCHK(c, dr.down(results, n));
    if (status) HIPCHK(c, dst.down(status, 4 * n));
    return MBLS_OK;
}
// what a call over a message list (mbls_verify_multiple*_shared_msgs: the description's ms then describes the n_msgs LISTED messages, set i's is message d_idx[i])
// or over a resident table (the _msgtable entries: d_idx holds TABLE indices) derives under the context's lock -- vm_shared_plan_and_reserve sets every field
struct vm_shared {
    mbls_shared_msgs_plan sp;          // the list hash (plan_shared)
    mbls_vm_shared_msgs_plan vp;       // the route (plan_vm_shared)
    uint64_t shadow_first = 0;         // the _locate entries: the first shadow item, behind phase one's workspace (mbls_vsl.h)
    // the span key source under a split (mbls_vcs.h): workspace items behind what the call plans today (set by the caller); base_items: that figure
    uint64_t extra_items = 0, base_items = 0;
    // what the grouping runs over (T) and what sizes the Miller phase (bound): the list both times, or the table as it is then and the bound on the named entries
    // (mbls_vmt.h); the table's buffers
    uint64_t T = 0, bound = 0; const uint32_t* tab = nullptr; uint64_t tstride = 0; const uint32_t* flags = nullptr;
};
// the message phase of the shared-message entries on stream s_msg: the list is hashed once into the context's table (the existing path of section 5d); the
// per-set route then gives every set its point (k_h_gather), the grouped route reads the table from its Miller items (k_vms_heads)
static int vm_shared_message_phase(mbls_ctx* c, mbls_ws ws, const vm_call& d, const vm_shared& sh, hipStream_t s_msg) {
    const uint64_t n = d.n;
    if (d.mt) {        // a resident table: nothing to hash; the per-set route gathers straight from it (the grouped route reads it from its Miller items, k_vmt_heads)
        if (sh.vp.route == MBLS_VM_ROUTE_PER_SET)
            hipLaunchKernelGGL(k_h_gather, dim3((unsigned)((n + MBLS_HB - 1) / MBLS_HB)), dim3(MBLS_HB), 0, s_msg, ws, sh.tab, sh.tstride, sh.flags, d.ms.d_idx, sh.T, c->d_status, n);
        return MBLS_OK;
    }
    const int rc = shared_hash_list(c, sh.sp, d.ms.d_msgs, d.ms.msg_len, d.ms.d_moff, d.ms.n_msgs, s_msg); if (rc) return rc;
    if (sh.vp.route == MBLS_VM_ROUTE_PER_SET)
        hipLaunchKernelGGL(k_h_gather, dim3((unsigned)((n + MBLS_HB - 1) / MBLS_HB)), dim3(MBLS_HB), 0, s_msg, ws, (const uint32_t*)c->d_htab, c->htab_cap,
                           (const uint32_t*)c->d_hflag, d.ms.d_idx, d.ms.n_msgs, c->d_status, n);
    return MBLS_OK;
}
static int vm_shared_plan_and_reserve(mbls_ctx* c, const vm_call& d, vm_shared& sh) {
    const uint64_t n = d.n;
    if (d.mt) {        // the table at the size it has now (the caller holds the context's lock); only the group arrays are reserved beside the workspace
        if (d.mt->c != c) ARGFAIL(c, "message table belongs to another context");
        sh.T = d.mt->size; sh.bound = vmt_bound(n, sh.T, d.named);
        sh.tab = d.mt->d_tab; sh.tstride = mtb_stride(d.mt->cap); sh.flags = d.mt->d_flag;
        memset(&sh.sp, 0, sizeof(sh.sp));
        plan_vm_msgtable(ctx_limits(c), n, sh.T, d.named, c->vm_grouping, d.longest, &sh.vp);
        const bool grouped = sh.vp.route == MBLS_VM_ROUTE_GROUPED;
        sh.shadow_first = vsl_shadow_first(n, sh.bound, grouped, 0);
        sh.base_items = d.locate ? vsl_workspace_items(n, sh.bound, grouped, 0) : sh.vp.workspace_items;
        const int rc = mbls_ctx_reserve(c, sh.base_items + sh.extra_items); if (rc) return rc;
        return reserve_groups(c, sh.T);
    }
    sh.T = sh.bound = d.ms.n_msgs;
    plan_shared(ctx_limits(c), n, d.ms.n_msgs, false, false, &sh.sp);
    plan_vm_shared(ctx_limits(c), n, d.ms.n_msgs, c->vm_grouping, d.longest, &sh.vp);
    const bool grouped = sh.vp.route == MBLS_VM_ROUTE_GROUPED;
    sh.shadow_first = vsl_shadow_first(n, d.ms.n_msgs, grouped, sh.sp.list_workspace_items);
    int rc = mbls_ctx_reserve(c, d.locate ? vsl_workspace_items(n, d.ms.n_msgs, grouped, sh.sp.list_workspace_items) : sh.vp.workspace_items); if (rc) return rc;
    return reserve_msgs(c, d.ms.n_msgs);
}
// the committee key source of mbls_verify_multiple_committee_msgtable* (one descriptor word and one bitfield per set, mbls_vmc.h) and its span form (mbls_vcs.h):
// the stride of a set's index list, and of a set's region of the span scratch
static uint64_t keys_list_stride(const keysrc& ks) { return ks.cmax ? ks.cmax : 1; }
static uint64_t keys_span_stride(const keysrc& ks) { return cms_stride(ks.bits_stride, ks.cmax); }
// for spans, the split factor of the call's key phase (it sizes the workspace: asked before that is reserved)
static uint32_t vm_committee_split(const mbls_ctx* c, const keysrc& ks, uint64_t n) {
    const mbls_limits L = ctx_limits(c);
    return ks.span ? vcs_split(n, keys_span_stride(ks), &L, c->vm_span_split) : 1u;
}
// The span key phase of verify_multiple_impl and vbg_impl on stream s: every set's two lists and record into the span scratch (reserve_committee_span), then the
// span key sum into the sets' APK slots -- one lane per set, or under a split (P > 1) one lane per chunk of a list, whose partial sums take the workspace items
// [partial_first, partial_first + 2 P n) and whose status words the same range of the context's words, and one combining lane per set. The sets' words: st_set.
static void vm_span_key_phase(mbls_ctx* c, mbls_ws ws, const keysrc& ks, uint64_t n, uint32_t P, uint64_t partial_first, uint32_t* st_set, hipStream_t s) {
    const uint64_t ls = keys_span_stride(ks);
    mbls_vcs_launch_expand(ks.d_crecs, ks.ccount, ks.d_members, ks.d_cmt_ids, ks.n_cmt_ids, ks.d_cmt_span_off, ks.d_bits, ks.bits_stride, c->cmt_route_mode,
                           c->d_cms_list, ls, c->d_cms_rec, n, s);
    if (P > 1u)
        mbls_vcs_launch_split(ws, partial_first, P, ks.d_recs, ks.tsize, c->d_cms_list, ls, c->d_cms_rec, ks.d_crecs, ks.d_cmt_ids, ks.d_cmt_span_off,
                              c->d_status + partial_first, st_set, n, s);
    else
        mbls_vcs_launch_aggregate(ws, ks.d_recs, ks.tsize, c->d_cms_list, ls, c->d_cms_rec, ks.d_crecs, ks.d_cmt_ids, ks.d_cmt_span_off, c->d_cms_park, c->cms_items,
                                  st_set, n, s);
}
// The key source of an entry that named its handle alone (keys_in_table, keys_in_committees, keys_in_committee_span), read at the sizes the handle has now (the
// caller holds the context's lock) with the checks of keys_of_table / keys_of_committees (one context, key table alive, bits_stride, alignment of device
// bitfields) / keys_of_committee_span (no bound between bits_stride and the largest committee -- every set's M is checked on its own)
static int vm_keys_resolve(mbls_ctx* c, keysrc* ks, bool device_bits) {
    if (ks->span) {
        const int rk = keys_of_committee_span(c, ks->cmt, ks->d_cmt_ids, ks->n_cmt_ids, ks->d_cmt_span_off, ks->d_bits, ks->bits_stride, device_bits, ks); if (rk) return rk;
        if (ks->ccount > (uint64_t)MBLS_VMC_SINGLE_KEY) ARGFAIL(c, "committee ids have 31 bits beside single-key sets");
        return MBLS_OK;
    }
    if (ks->committee) return keys_of_committees(c, ks->cmt, ks->d_cmt_idx, ks->d_bits, ks->bits_stride, device_bits, ks);
    if (ks->indexed) return keys_of_table(c, ks->tab, ks->d_idx, ks->d_off, ks);
    return MBLS_OK;
}
// the host entries' statement of "malformed" (what k_vcs_expand rejects per set refuses the whole call here), and a single-key index that names no key
static int vm_committee_span_sets_ok(mbls_ctx* c, const host_committees& hc, const keysrc& ks, uint64_t n) {
    if (!hc.cmt_off || (hc.n_cmt_ids && !hc.cmt_ids) || (hc.bits_stride && !hc.bits)) ARGFAIL(c, "null buffer");
    for (uint64_t i = 0; i < n; i++) {
        uint32_t q = 0;
        if (!cms_range_ok(hc.cmt_off[i], hc.cmt_off[i + 1], hc.n_cmt_ids, &q)) ARGFAIL(c, "cmt_off must be non-decreasing, inside cmt_ids, at most MBLS_SPAN_MAX_COMMITTEES ids per set");
        const uint32_t* ids = hc.cmt_ids + hc.cmt_off[i];
        if (q == 1u && vcs_is_single(q, ids[0])) {
            if (vcs_single_names_nothing(ids[0], ks.tsize)) ARGFAIL(c, "cmt_ids names no key of the key table");
            continue;
        }
        uint64_t M = 0;
        for (uint32_t u = 0; u < q; u++) {
            if (!vcs_id_ok(ids[u], ks.ccount)) ARGFAIL(c, "cmt_ids names no committee of the table");
            M += hc.t->sizes[ids[u]];
        }
        if (!cms_field_ok(M, hc.bits_stride)) ARGFAIL(c, "bits_stride does not cover a set's committees");
    }
    return MBLS_OK;
}
static int verify_multiple_impl(mbls_ctx* c, const vm_call& d, void* stream) {
    // the key source is one of five (vm_key_kind); the committee kinds run over a resident message table only
    // d.sigs_resident: k_sig (decode + subgroup test) has run over these signatures on this workspace and the host has seen every one pass: d.d_sigs is not read.
    // d.hash_enqueued (batches whose chains run side by side only): the message phase is already on the context's message stream.
    if (!c || (!d.d_result && !d.d_partial)) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    const uint64_t n = d.n; const keysrc& ks = d.ks; const int keys = vm_key_kind(d);
    const bool committee = keys == VM_KEYS_SPAN || keys == VM_KEYS_COMMITTEE, shared = d.ms.indexed();
    uint8_t* const d_result = d.d_result; uint32_t* const d_partial = d.d_partial; const uint64_t* const d_rands = d.d_rands;
    vm_shared sh;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (n == 0 && d_partial) {     // an empty shard contributes (1, infinity, no status bits)
        mbls_ws none; none.w = nullptr; none.stride = 0;
        hipLaunchKernelGGL(k_vm_export, dim3(1), dim3(WG), 0, s, none, (const uint32_t*)nullptr, 1, d_partial);
        HIPCHK(c, hipGetLastError());
        return MBLS_OK;
    }
    if (n == 0) {     // empty iterator: S' = infinity, product of no pairings = 1 -> e(inf, -G1) = 1 -> true
        HIPCHK(c, hipMemsetAsync(d_result, 1, 1, s));
        if (d.d_status_or) HIPCHK(c, hipMemsetAsync(d.d_status_or, 0, 4, s));
        return MBLS_OK;
    }
    if (!d_rands) ARGFAIL(c, "verify_multiple without blinding scalars is forgeable: rands must not be NULL");
    if ((!d.d_sigs && !d.sigs_resident) || (!d.ms.d_msgs && d.ms.msg_len && !d.ms.d_moff && !(shared && !d.ms.n_msgs))) ARGFAIL(c, "null buffer");
    if (d.mt && d_partial) ARGFAIL(c, "the shard form takes per-set messages only");
    // batches of at most half a round: two lanes per message in the message phase (items [0, 2 n), slots no other chain touches)
    const bool pair_hash = !shared && n <= c->split_max_items && 2 * n <= c->round_items;
    // a shared list: the workspace (sets, Miller items, positions, the list's own hash) and the table are reserved here, once, before the first kernel
    // the span form of the committee source under a split: the partial sums' workspace items behind the call's own (mbls_vcs.h)
    const uint32_t span_split = committee && shared ? vm_committee_split(c, ks, n) : 1u;
    if (committee && shared) sh.extra_items = vcs_extra_items(n, span_split);
    int rc = shared ? vm_shared_plan_and_reserve(c, d, sh) : mbls_ctx_reserve(c, pair_hash ? 2 * n : n); if (rc) return rc;
    // the committee source: the sets' index lists, count and route words for all n sets (spans: their regions, records and parked points), reserved here with the
    // workspace (grow-only: nothing when mbls_ctx_reserve_committee[_span]_items or the first half of an _rng call has been there)
    if (committee) {
        if (!d.mt || d_partial) ARGFAIL(c, "internal: the committee source runs over a resident message table only");
        rc = ks.span ? reserve_committee_span(c, n, keys_span_stride(ks)) : reserve_committee(c, n, ks.cmax); if (rc) return rc;
    }
    const bool grouped = shared && sh.vp.route == MBLS_VM_ROUTE_GROUPED;
    const uint64_t n_miller = grouped ? sh.vp.miller_items : n;
    const bool loc = shared && d.locate;
    const uint64_t shf = loc ? sh.shadow_first : 0;                // locate mode: the first shadow item; the candidate flags (cap >= 2 n words)
    uint32_t* const cand = c->d_status + vsl_flags_first(n);
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    rc = ws_acquire(c, s); if (rc) return rc;
    // a resident message table: its last append and the key table's are awaited on the caller's stream HERE, before anything is enqueued on a side stream -- every
    // stream of the call forks from s behind them, and no fallible step is left once a side stream has work
    const bool over_table = d.mt != nullptr;
    if (over_table) { rc = msgtable_acquire(c, d.mt, s); if (rc) return rc; if (keys == VM_KEYS_TABLE) { rc = table_acquire(c, ks.tab, s); if (rc) return rc; } }
    if (committee) { rc = committees_acquire(c, ks.cmt, s); if (rc) return rc; rc = table_acquire(c, ks.tab, s); if (rc) return rc; }
    if (loc) {
        HIPCHK(c, hipMemsetAsync(d.d_set_results, 0, n, s));      // fail closed
        if (d.d_set_status) HIPCHK(c, hipMemsetAsync(d.d_set_status, 0, 4 * n, s));
        HIPCHK(c, hipMemsetAsync(cand, 0, 4 * n, s));
    }
    HIPCHK(c, hipMemsetAsync(c->d_scalar, 0, 64, s));
    if (!d.sigs_resident) HIPCHK(c, hipMemsetAsync(c->d_status, 0, 4 * n, s));      // (resident: cleared before k_sig, and the message phase may be writing its bits)
    if (d_partial) HIPCHK(c, hipMemsetAsync(d_partial, 0, MBLS_VM_PARTIAL_BYTES, s));       // not a record until k_vm_export has spoken
    else HIPCHK(c, hipMemsetAsync(d_result, 0, 1, s));                      // false until the tail kernel has spoken (fail closed)
    // Three independent chains: keys (aggregate, [r]apk), signatures (decode, subgroup check, [r]sig, sum tree), messages (hash). Below
    // half a round of lanes each of them leaves at least half the SIMDs idle, so they run side by side on the context's streams and join before
    // the Miller loops (2^15 sets: 13.4 ms instead of 18.3 one after the other); closer to a full round the three chains only get in each
    // other's way (65 535 sets: 24.7 ms side by side, 21.2 in a row) and stay on the caller's stream.
    const bool fork = 2 * n <= c->round_items;
    hipStream_t s_sig = fork ? c->hs_b : s, s_msg = fork ? c->hs_c : s;
    if (fork) { HIPCHK(c, hipEventRecord(c->hs_ev, s)); HIPCHK(c, hipStreamWaitEvent(s_sig, c->hs_ev, 0)); HIPCHK(c, hipStreamWaitEvent(s_msg, c->hs_ev, 0)); }
    // side by side, the message phase is the chain the sets' Miller loops wait for: it is ENQUEUED first (behind the ~20 launches of the signature chain's sum tree
    // it started 0.26 ms late: 2^14 sets 9.47 -> 9.2 ms)
    const bool hash_first = fork && !d.hash_enqueued;
    auto message_phase = [&]() -> int {
        if (shared) return vm_shared_message_phase(c, ws, d, sh, s_msg);
        launch_hash(c, ws, d.ms.d_msgs, d.ms.msg_len, d.ms.d_moff, c->d_status, n, s_msg, pair_hash); return MBLS_OK;
    };
    if (hash_first) { rc = message_phase(); if (rc) return rc; }
    if (keys == VM_KEYS_SPAN) {   // sets given by committee span, or by one key index (mbls_vcs.h): every set's two lists and record, then the span key sum -- one lane per
        // set, or under a split one lane per chunk of a list (workspace items and status words behind the call's own and its extra lane) and one combining lane per set
        vm_span_key_phase(c, ws, ks, n, span_split, sh.base_items + 1, c->d_status, s);
    } else if (keys == VM_KEYS_COMMITTEE) {       // sets given by committee and bitfield, or by one key index (mbls_vmc.h): every set's list, then the indexed key sum over it with the complement's fix-up
        const uint64_t ls = keys_list_stride(ks);
        uint32_t* const cnt = c->d_cmt_cnt; uint32_t* const route = c->d_cmt_cnt + c->cmt_items;
        hipLaunchKernelGGL(k_vmc_expand, dim3((unsigned)n), dim3(WG), 0, s, ks.d_crecs, ks.ccount, ks.d_members, ks.d_cmt_idx, ks.d_bits, ks.bits_stride, c->cmt_route_mode,
                           c->d_cmt_list, ls, cnt, route, n);
        hipLaunchKernelGGL(k_aggregate_vmc_d, dim3(nblk(n)), dim3(WG), 0, s, ws, ks.d_recs, ks.tsize, (const uint32_t*)c->d_cmt_list, ls, (const uint32_t*)cnt, (const uint32_t*)route,
                           ks.d_crecs, ks.d_cmt_idx, c->d_status, n);
    } else if (keys == VM_KEYS_TABLE) {      // sets given by indices into a resident key table: the indexed key sum (the keys were decoded and validated once)
        if (!over_table) { rc = table_acquire(c, ks.tab, s); if (rc) return rc; }
        hipLaunchKernelGGL(k_aggregate_indexed_d, dim3(nblk(n)), dim3(WG), 0, s, ws, ks.d_recs, ks.tsize, ks.d_idx, ks.d_off, d.k, MBLS_MODE_VERIFY, c->d_status, n);
    } else if (keys == VM_KEYS_WIRE)    // sets given by their wire-format keys: AggregatePublicKey::aggregate on the device first (src/aggregates.rs:29-39)
        launch_aggregate(ws, ks.d_pks, ks.d_off, d.k, ks.fmt, MBLS_MODE_VERIFY, c->d_status, n, s);
    hipLaunchKernelGGL(k_blind_g1_d, dim3(nblk(n)), dim3(WG), 0, s, ws, keys == VM_KEYS_APKS ? d.d_apks : (const uint8_t*)nullptr, d_rands, c->d_status, n);
    // one Miller loop per message: count, scan, scatter and the per-message sums of the blinded keys follow the keys on their stream (beside the list's hash and
    // the signature chain where the chains run side by side); the heads wait for the table further down
    const uint64_t pbase = grouped ? vms_position_base(n, sh.bound) : 0;
    uint32_t* const g_cnt = c->d_hgrp; uint32_t* const g_cur = c->d_hgrp + c->hgrp_cap; uint32_t* const g_off = c->d_hgrp + 2 * c->hgrp_cap;
    uint32_t* const g_flag = c->d_hgrp + 3 * c->hgrp_cap; uint32_t* const g_roff = c->d_hgrp + 4 * c->hgrp_cap; uint32_t* const g_named = c->d_hgrp + 5 * c->hgrp_cap;
    if (grouped) {
        const uint64_t M = sh.T;
        HIPCHK(c, hipMemsetAsync(g_cnt, 0, 4 * (M + 1), s)); HIPCHK(c, hipMemsetAsync(g_cur, 0, 4 * (M + 1), s)); HIPCHK(c, hipMemsetAsync(c->d_vmap, 0xFF, 4 * n, s));
        hipLaunchKernelGGL(k_vms_count, dim3(nblk(n)), dim3(WG), 0, s, d.ms.d_idx, M, n, g_cnt, c->d_status);
        hipLaunchKernelGGL(k_vms_scan, dim3(1), dim3(MBLS_VMS_SCAN_LANES), 0, s, (const uint32_t*)g_cnt, M, g_off);
        if (loc) hipLaunchKernelGGL(k_vsl_keep_key, dim3(nblk(n)), dim3(WG), 0, s, ws, n, shf);      // [r_i] apk_i -> A(i), before heads and trees run over the sets' items
        hipLaunchKernelGGL(k_vms_scatter, dim3(nblk(n)), dim3(WG), 0, s, ws, d.ms.d_idx, M, n, (const uint32_t*)g_off, g_cur, c->d_vmap, pbase);
        mbls_ws wp = ws; wp.w += pbase;
        uint64_t half = 1;
        for (uint32_t l = 0; l < sh.vp.tree_levels; l++, half *= 2)
            hipLaunchKernelGGL(k_g1_seg_tree_d, dim3(nblk(n)), dim3(WG), 0, s, wp, (const uint32_t*)c->d_vmap, (const uint32_t*)g_off, M, n, half);
        if (over_table) {       // the entries the call names, in increasing table index; D = g_roff[M] stays on the device (mbls_vmt.h)
            HIPCHK(c, hipMemsetAsync(g_roff, 0, 4 * (M + 1), s));
            if (M) {
                hipLaunchKernelGGL(k_vmt_flag, dim3(nblk(M)), dim3(WG), 0, s, (const uint32_t*)g_cnt, M, g_flag);
                hipLaunchKernelGGL(k_vms_scan, dim3(1), dim3(MBLS_VMS_SCAN_LANES), 0, s, (const uint32_t*)g_flag, M, g_roff);
                hipLaunchKernelGGL(k_vmt_named, dim3(nblk(M)), dim3(WG), 0, s, (const uint32_t*)g_flag, (const uint32_t*)g_roff, M, g_named);
            }
        }
    }
    const uint32_t* const d_live = grouped && over_table ? g_roff + sh.T : nullptr;      // the Miller items that have a pair at all
    // small batches (their Miller loops run one WAVE per pair, see npairing_finish): the signature chain is what the call waits for -- two lanes per signature
    if (2 * n <= c->coop_max_items)
        hipLaunchKernelGGL(k_blind_sig2_d, dim3(nblk(2 * n)), dim3(WG), 0, s_sig, ws, d.sigs_resident ? (const uint8_t*)nullptr : d.d_sigs, d_rands, c->d_status, n);
    else
        hipLaunchKernelGGL(k_blind_sig_d, dim3(nblk(n)), dim3(WG), 0, s_sig, ws, d.sigs_resident ? (const uint8_t*)nullptr : d.d_sigs, d_rands, c->d_status, n);
    // locate mode: ([r_i] sig_i, -G1) -> the set's shadow item (grouped: B(i)), before the sum tree runs over slot S
    if (loc) hipLaunchKernelGGL(k_vml_keep_sig, dim3(nblk(n)), dim3(WG), 0, s_sig, ws, n, grouped ? shf + n : shf);
    const bool side_s_chain = !fork && s != c->hs_b;                  // the sum tree waits for the product tree's company (npairing_finish)
    if (!side_s_chain) g2_tree(c, ws, n, s_sig);
    if (fork) {     // S is complete: its Miller loop runs on one wave beside the other chains and the sets' Miller loops (most SIMDs are idle)
        HIPCHK(c, hipEventRecord(c->hs_ev2, s_sig));                 // the status bits and S exist
        if (!d_partial)                                              // (a shard's S joins the other shards' first: mbls_verify_multiple_finish_device)
            coop_run(c, COOP_SMILLER, ws, (uint64_t)0, (uint64_t)1, (uint64_t)0, (uint64_t)1, (uint32_t*)nullptr, (uint8_t*)nullptr, COOP_RES_ITEM, s_sig);
        HIPCHK(c, hipEventRecord(c->hs_ev, s_sig));                  // ... and its Miller value (awaited just before the tail)
    }
    if (!(d.hash_enqueued && fork) && !hash_first) { rc = message_phase(); if (rc) return rc; }
    if (fork) {      // the sets' Miller loops need the keys (this stream) and the messages; the signature chain is awaited before the tail (hs_ev)
        HIPCHK(c, hipEventRecord(c->hs_ev3, s_msg));
        HIPCHK(c, hipStreamWaitEvent(s, c->hs_ev3, 0));
    } else
        hipLaunchKernelGGL(k_status_or, dim3(nblk(n)), dim3(WG), 0, s, c->d_status, n, c->d_scalar);
    if (grouped && over_table)
        hipLaunchKernelGGL(k_vmt_heads, dim3((unsigned)((n_miller + MBLS_HB - 1) / MBLS_HB)), dim3(MBLS_HB), 0, s, ws, sh.tab, sh.tstride, sh.flags, sh.T, (const uint32_t*)g_off,
                           (const uint32_t*)g_named, d_live, n_miller, pbase, c->d_scalar);
    else if (grouped)     // the table is complete: every Miller item gets its message's point and its group's key (a bad listed range some set names: the status word)
        hipLaunchKernelGGL(k_vms_heads, dim3((unsigned)((n_miller + MBLS_HB - 1) / MBLS_HB)), dim3(MBLS_HB), 0, s, ws, (const uint32_t*)c->d_htab, c->htab_cap,
                           (const uint32_t*)c->d_hflag, (const uint32_t*)g_off, (const uint32_t*)g_cnt, d.ms.n_msgs, n_miller, pbase, c->d_scalar);
    // a set whose signature is outside G2 (reference src/aggregates.rs:274-276), an undecodable member or a zero scalar makes the tail
    // answer false: the status bits are folded in on the device, the call only enqueues
    rc = npairing_finish(c, n_miller, s, d_result, fork ? c->hs_ev : nullptr, fork, d_partial, side_s_chain, n, loc && !grouped ? shf : 0, d_live); if (rc) return rc;
    if (d.d_status_or) HIPCHK(c, hipMemcpyAsync(d.d_status_or, c->d_scalar, 4, hipMemcpyDeviceToDevice, s));
    if (loc && grouped) {      // phase two, enqueued whatever the verdict is: mark through msg_idx (candidates get their H), both pairs' Miller loops, product, final
        mbls_ws wsa = ws; wsa.w += shf;
        hipLaunchKernelGGL(k_vsl_mark, dim3(nblk(n)), dim3(WG), 0, s, wsa, over_table ? sh.tab : (const uint32_t*)c->d_htab, over_table ? sh.tstride : c->htab_cap,
                           over_table ? sh.flags : (const uint32_t*)c->d_hflag, d.ms.d_idx, sh.T, n, (const uint32_t*)c->d_status, (const uint8_t*)d_result, cand, d.d_set_results, d.d_set_status);
        vsl_examine(c, ws, n, shf, true, c->d_status, cand, d.d_set_results, d.d_set_status, s);
        HIPCHK(c, hipGetLastError());
    } else if (loc) {          // the per-set route: the scheme of mbls_verify_multiple_batches_locate* with the call as the one batch that owns every set
        hipLaunchKernelGGL(k_vml_mark, dim3(nblk(n)), dim3(WG), 0, s, ws, (const uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t)n, (uint64_t)1, n,
                           (const uint32_t*)c->d_status, (const uint32_t*)nullptr, (const uint8_t*)d_result, cand, d.d_set_results, d.d_set_status, shf);
        vsl_examine(c, ws, n, shf, false, c->d_status, cand, d.d_set_results, d.d_set_status, s);
        HIPCHK(c, hipGetLastError());
    }
    return ws_release(c, s);
}
// verify_multiple over sets named by indices into a resident key table (the deployment's form: validator keys are decoded once, a set is a list of
// validator indices): set i owns indices [d_offsets[i], d_offsets[i+1]) of d_key_idx, or k each. d_partial (optional) instead of d_result: the shard form.
extern "C" int mbls_verify_multiple_sets_indexed_device(mbls_ctx* c, const mbls_keytable* t, const uint8_t* d_sigs, const uint32_t* d_key_idx, const uint32_t* d_offsets,
        uint32_t k, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff, const uint64_t* d_rands, uint64_t n, uint8_t* d_result, uint32_t* d_status_or,
        uint8_t* d_partial, void* stream) {
    if (!c || !t || (!d_result && !d_partial)) return MBLS_ERR_ARGUMENT;
    if (n && !d_key_idx) return MBLS_ERR_ARGUMENT;
    if (((uintptr_t)d_partial) & 3) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    keysrc ks; const int rk = keys_of_table(c, t, d_key_idx, d_offsets, &ks); if (rk) return rk;
    const vm_call d = vm_sets(d_sigs, d_rands, n).keys(ks, k).msgs(msgs_per_item(d_msgs, msg_len, d_moff));
    return verify_multiple_impl(c, d_partial ? d.out_partial((uint32_t*)d_partial) : d.out(d_result, d_status_or), stream);
}
// One shard of a verify_multiple that is spread over several devices or processes: everything up to the shard's
// Miller product and signature sum, left as one MBLS_VM_PARTIAL_BYTES record in device memory. Enqueues only.
extern "C" int mbls_verify_multiple_partial_device(mbls_ctx* c, const uint8_t* d_sigs, const uint8_t* d_apks, const uint8_t* d_pks, int pk_format,
        const uint32_t* d_pk_offsets, uint32_t k, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff, const uint64_t* d_rands, uint64_t n,
        uint8_t* d_partial, void* stream) {
    if (!c || !d_partial) return MBLS_ERR_ARGUMENT;
    if (n && !d_apks && !d_pks) return MBLS_ERR_ARGUMENT;
    if (!d_apks && pk_format != MBLS_PK_COMPRESSED && pk_format != MBLS_PK_UNCOMPRESSED) return MBLS_ERR_ARGUMENT;
    if (((uintptr_t)d_partial) & 3) return MBLS_ERR_ARGUMENT;
    const vm_call d = vm_sets(d_sigs, d_rands, n).msgs(msgs_per_item(d_msgs, msg_len, d_moff)).out_partial((uint32_t*)d_partial);
    return verify_multiple_impl(c, d_apks ? d.keys_apks(d_apks) : d.keys(keys_wire(d_pks, pk_format, d_pk_offsets), k), stream);
}
// The exchange step's second half: G records (the shards' in any fixed order -- every participant that uses the same order computes the same
// bool) -> product and sum trees over the records, then the tail of the one-device check: the Miller loop of (S, -G1), the product, ONE final
// exponentiation, the comparison, the status bits (program vmtail; reference src/aggregates.rs:307-315). Enqueues only.
extern "C" int mbls_verify_multiple_finish_device(mbls_ctx* c, const uint8_t* d_partials, uint64_t G, uint8_t* d_result, uint32_t* d_status_or, void* stream) {
    if (!c || !d_result) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (G == 0) {      // no shards: the empty iterator
        HIPCHK(c, hipMemsetAsync(d_result, 1, 1, s));
        if (d_status_or) HIPCHK(c, hipMemsetAsync(d_status_or, 0, 4, s));
        return MBLS_OK;
    }
    if (!d_partials || (((uintptr_t)d_partials) & 3)) ARGFAIL(c, "null or unaligned records");
    int rc = mbls_ctx_reserve(c, G); if (rc) return rc;
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    rc = ws_acquire(c, s); if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_scalar, 0, 64, s));
    HIPCHK(c, hipMemsetAsync(d_result, 0, 1, s));
    hipLaunchKernelGGL(k_vm_import, dim3(nblk(G)), dim3(WG), 0, s, ws, (const uint32_t*)d_partials, G, c->d_scalar);
    f12_tree(c, ws, G, s);
    g2_tree(c, ws, G, s);
    coop_run(c, COOP_VMTAIL, ws, (uint64_t)0, (uint64_t)1, (uint64_t)0, (uint64_t)1, c->d_scalar, d_result, COOP_RES_BATCH, s);
    HIPCHK(c, hipGetLastError());
    if (d_status_or) HIPCHK(c, hipMemcpyAsync(d_status_or, c->d_scalar, 4, hipMemcpyDeviceToDevice, s));
    return ws_release(c, s);
}
extern "C" int mbls_verify_multiple_aggregate_signatures_device(mbls_ctx* c, const uint8_t* d_sigs, const uint8_t* d_apks, const uint8_t* d_msgs,
        uint32_t msg_len, const uint64_t* d_moff, const uint64_t* d_rands, uint64_t n, uint8_t* d_result, uint32_t* d_status_or, void* stream) {
    if (!c) return MBLS_ERR_ARGUMENT;
    if (n && !d_apks) return MBLS_ERR_ARGUMENT;
    return verify_multiple_impl(c, vm_sets(d_sigs, d_rands, n).keys_apks(d_apks).msgs(msgs_per_item(d_msgs, msg_len, d_moff)).out(d_result, d_status_or), stream);
}
extern "C" int mbls_verify_multiple_sets_device(mbls_ctx* c, const uint8_t* d_sigs, const uint8_t* d_pks, int pk_format, const uint32_t* d_pk_offsets,
        uint32_t k, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff, const uint64_t* d_rands, uint64_t n, uint8_t* d_result,
        uint32_t* d_status_or, void* stream) {
    if (!c) return MBLS_ERR_ARGUMENT;
    if (pk_format != MBLS_PK_COMPRESSED && pk_format != MBLS_PK_UNCOMPRESSED) return MBLS_ERR_ARGUMENT;
    if (n && !d_pks) return MBLS_ERR_ARGUMENT;
    return verify_multiple_impl(c, vm_sets(d_sigs, d_rands, n).keys(keys_wire(d_pks, pk_format, d_pk_offsets), k).msgs(msgs_per_item(d_msgs, msg_len, d_moff))
                                       .out(d_result, d_status_or), stream);
}
extern "C" int mbls_verify_multiple_aggregate_signatures(mbls_ctx* c, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs,
        uint32_t msg_len, const uint64_t* moff, const uint64_t* rands, size_t n) {
    if (!c) return 0;
    if (n == 0) return 1;
    if (moff && !msg_offsets_ok(moff, n)) return 0;
    const uint64_t msg_first = moff ? moff[0] : 0;
    const size_t msg_total = moff ? (size_t)(moff[n] - moff[0]) : (size_t)msg_len * n;
    if (!sigs96 || !apks96 || !rands || (!msgs && msg_total)) return 0;
    mbls_lock lk(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return 0;
    sbuf ds(c, 0), da(c, 1), dm(c, 2), dr(c, 3), dmo(c, 6), dres(c, 4);
    if (ds.up(sigs96, 96 * n) != hipSuccess || da.up(apks96, 96 * n) != hipSuccess || dm.up(msgs ? msgs + msg_first : nullptr, msg_total) != hipSuccess ||
        dr.up(rands, 8 * n) != hipSuccess || (moff && dmo.up(moff, 8 * (n + 1)) != hipSuccess) || dres.alloc(8) != hipSuccess) return 0;
    if (mbls_verify_multiple_aggregate_signatures_device(c, ds.as<uint8_t>(), da.as<uint8_t>(), dm.as<uint8_t>() - msg_first, msg_len,
                                                         moff ? dmo.as<uint64_t>() : nullptr, dr.as<uint64_t>(), n, dres.as<uint8_t>(), nullptr, c->hs_a)) return 0;
    uint8_t r = 0;
    if (hipStreamSynchronize(c->hs_a) != hipSuccess) return 0;
    c->ws_pending = false;
    if (dres.down(&r, 1) != hipSuccess) return 0;
    return r;
}
// The reference's own shape (src/aggregates.rs:261-316): its loop tests set i's signature for the subgroup (:272-275) BEFORE it draws rand[i] from the caller's
// generator (:280-287) and returns at the first signature outside G2 -- so a rejected batch leaves the generator after exactly as many draws as sets came before
// the bad one. One call does the same: the signatures are decoded and tested first (k_sig, beside the message phase when the batch leaves room), the host reads
// the verdicts, `draw` is asked for exactly the scalars the reference would have drawn, and what follows skips the second subgroup test (the points are in the slots).
// The two halves of that call, shared with the several-device form (mbls_multi_verify_multiple_aggregate_signatures_rng): phase 1 stages a shard's sets, decodes and
// tests its signatures (they stay in the workspace), starts the message phase and reads the verdicts back; phase 2 takes the scalars and runs the rest -- up to the
// bool (d_partial == nullptr) or up to the shard's record. The caller holds the context's lock across both.
struct vm_rng_stage {
    sbuf ds, da, dm, dr, dmo, dout, dmi, dci, dso;  // (dci: the sets' descriptor words of the committee form, whose bitfields travel in da -- it has no aggregate keys;
                                                    //  dso: the span form's offsets, its ids in dci)
    const uint8_t* d_msgs = nullptr; const uint64_t* d_moff = nullptr;
    vm_rng_stage(mbls_ctx* c) : ds(c, 0), da(c, 1), dm(c, 2), dr(c, 3), dmo(c, 6), dout(c, 4), dmi(c, 7), dci(c, 10), dso(c, 5) {}
};
static void vm_rng_drain(mbls_ctx* c) { (void)hipStreamSynchronize(c->hs_a); (void)hipStreamSynchronize(c->hs_b); (void)hipStreamSynchronize(c->hs_c); c->ws_pending = false; }
// the signature half of an _rng call on stream s (fork: on the context's signature stream, with the message stream forked beside it): the sets' status words
// cleared, the signatures decoded and tested -- they stay in the workspace; the verdicts are complete on that stream
static int vm_rng_signatures(mbls_ctx* c, mbls_ws ws, const uint8_t* d_sigs, uint64_t n, hipStream_t s, bool fork) {
    hipStream_t s_sig = fork ? c->hs_b : s;
    if (hipMemsetAsync(c->d_status, 0, 4 * n, s) != hipSuccess) return MBLS_ERR_DEVICE;
    if (fork) { (void)hipEventRecord(c->hs_ev, s); (void)hipStreamWaitEvent(c->hs_b, c->hs_ev, 0); (void)hipStreamWaitEvent(c->hs_c, c->hs_ev, 0); }
    if (2 * n <= c->coop_max_items) hipLaunchKernelGGL(k_sig2, dim3(nblk(2 * n)), dim3(WG), 0, s_sig, ws, d_sigs, c->d_status, n);
    else hipLaunchKernelGGL(k_sig, dim3(nblk(n)), dim3(WG), 0, s_sig, ws, d_sigs, c->d_status, n, 1);
    return MBLS_OK;
}
// h: the shard's own sets in host memory; its messages: the buffer the (absolute) offsets of moff[0 .. n] point into, or n x msg_len bytes -- over a list, the
// n_msgs LISTED messages, and the sets' indices are uploaded here. The committee forms (h.hc; no aggregate keys): the sets' words and bitfields are uploaded here
// and the list scratch of the whole call is reserved with the workspace. d: the call as its entry resolved it (key source, table, locate outputs); its device
// pointers are set here. -> MBLS_OK and st[0 .. n) (status words)
static int vm_rng_phase1(mbls_ctx* c, vm_rng_stage& g, const vm_host& h, size_t out_bytes, uint32_t* st, vm_call* d) {
    const size_t n = (size_t)h.n; const host_committees* const hc = h.hc; const uint64_t* const moff = h.ms.d_moff;
    const bool shared = h.ms.indexed();
    d->n = n;
    if (hipSetDevice(c->device) != hipSuccess) return MBLS_ERR_DEVICE;
    if (g.dout.alloc(out_bytes) != hipSuccess) return MBLS_ERR_DEVICE;
    if (n == 0) return MBLS_OK;
    const size_t nm = shared ? (size_t)h.ms.n_msgs : n;                     // messages the buffers describe
    const uint64_t msg_first = moff ? moff[0] : 0;
    const size_t msg_total = moff ? (size_t)(moff[nm] - moff[0]) : (size_t)h.ms.msg_len * nm;
    if (g.ds.up(h.sigs96, 96 * n) != hipSuccess || (!hc && g.da.up(h.apks96, 96 * n) != hipSuccess) ||
        g.dm.up(h.ms.d_msgs ? h.ms.d_msgs + msg_first : nullptr, msg_total) != hipSuccess || g.dr.alloc(8 * n) != hipSuccess ||
        (moff && g.dmo.up(moff, 8 * (nm + 1)) != hipSuccess)) return MBLS_ERR_DEVICE;
    if (hc && hc->span) {       // the ids take the descriptor words' slot, the span offsets one of their own
        if (g.da.up(hc->bits, (size_t)hc->bits_stride * n) != hipSuccess || g.dci.up(hc->cmt_ids, 4 * hc->n_cmt_ids) != hipSuccess ||
            g.dso.up(hc->cmt_off, 4 * (n + 1)) != hipSuccess) return MBLS_ERR_DEVICE;
        d->ks.d_bits = g.da.as<uint8_t>(); d->ks.d_cmt_ids = g.dci.as<uint32_t>(); d->ks.d_cmt_span_off = g.dso.as<uint32_t>();
    } else if (hc) {
        if (g.da.up(hc->bits, (size_t)hc->bits_stride * n) != hipSuccess || g.dci.up(hc->cmt_idx, 4 * n) != hipSuccess) return MBLS_ERR_DEVICE;
        d->ks.d_bits = g.da.as<uint8_t>(); d->ks.d_cmt_idx = g.dci.as<uint32_t>();
    } else d->d_apks = g.da.as<uint8_t>();
    d->ms = h.ms; d->ms.d_msgs = g.dm.as<uint8_t>() - msg_first; d->ms.d_moff = moff ? g.dmo.as<uint64_t>() : nullptr;
    if (shared) { if (g.dmi.up(h.ms.d_idx, 4 * n) != hipSuccess) return MBLS_ERR_DEVICE; d->ms.d_idx = g.dmi.as<uint32_t>(); }
    hipStream_t s = c->hs_a;
    const bool pair_hash = !shared && n <= c->split_max_items && 2 * n <= c->round_items, fork = 2 * n <= c->round_items;       // as verify_multiple_impl decides
    vm_shared sh;
    if (hc && shared) sh.extra_items = vcs_extra_items(n, vm_committee_split(c, d->ks, n));      // (the whole call's workspace, as verify_multiple_impl will ask for it)
    int rc = shared ? vm_shared_plan_and_reserve(c, *d, sh) : mbls_ctx_reserve(c, pair_hash ? 2 * n : n); if (rc) return rc;
    if (hc) { rc = hc->span ? reserve_committee_span(c, n, keys_span_stride(d->ks)) : reserve_committee(c, n, d->ks.cmax); if (rc) return rc; }
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    rc = ws_acquire(c, s); if (rc) return rc;
    if (d->mt) { rc = msgtable_acquire(c, d->mt, s); if (rc) return rc; }      // (before the fork: the message stream inherits the table's last append)
    hipStream_t s_sig = fork ? c->hs_b : s;
    if (vm_rng_signatures(c, ws, g.ds.as<uint8_t>(), n, s, fork)) { vm_rng_drain(c); return MBLS_ERR_DEVICE; }
    if (fork && shared) { rc = vm_shared_message_phase(c, ws, *d, sh, c->hs_c); if (rc) { vm_rng_drain(c); return rc; } }
    else if (fork) launch_hash(c, ws, d->ms.d_msgs, d->ms.msg_len, d->ms.d_moff, c->d_status, n, c->hs_c, pair_hash);       // the message phase does not wait for the host
    if (hipStreamSynchronize(s_sig) != hipSuccess || hipMemcpy(st, c->d_status, 4 * n, hipMemcpyDeviceToHost) != hipSuccess) { vm_rng_drain(c); return MBLS_ERR_DEVICE; }
    return MBLS_OK;
}
// rands[0 .. n): the shard's scalars. partial == false: the bool is left in g.dout (1 byte); true: the shard's record (MBLS_VM_PARTIAL_BYTES). Enqueues on hs_a.
static int vm_rng_phase2(mbls_ctx* c, vm_rng_stage& g, const uint64_t* rands, bool partial, const vm_call& d) {
    if (hipSetDevice(c->device) != hipSuccess) return MBLS_ERR_DEVICE;
    if (d.n && g.dr.up(rands, 8 * d.n) != hipSuccess) return MBLS_ERR_DEVICE;
    const vm_call h = d.second_half(g.dr.as<uint64_t>(), true);
    return verify_multiple_impl(c, partial ? h.out_partial(g.dout.as<uint32_t>()) : h.out(g.dout.as<uint8_t>(), nullptr), c->hs_a);
}
extern "C" int mbls_verify_multiple_aggregate_signatures_rng(mbls_ctx* c, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs,
        uint32_t msg_len, const uint64_t* moff, size_t n, mbls_scalar_source draw, void* user) {
    if (!c) return 0;
    if (n == 0) return 1;                                                   // empty iterator: true, the generator untouched
    if (!draw) return 0;
    if (moff && !msg_offsets_ok(moff, n)) return 0;
    const size_t msg_total = moff ? (size_t)(moff[n] - moff[0]) : (size_t)msg_len * n;
    if (!sigs96 || !apks96 || (!msgs && msg_total)) return 0;
    mbls_lock lk(c->mu);
    std::vector<uint64_t> rands; std::vector<uint32_t> st;
    try { rands.resize(n); st.resize(n); } catch (...) { return 0; }
    vm_rng_stage g(c); vm_call d;
    if (vm_rng_phase1(c, g, vm_host_sets(sigs96, n).keys_apks(apks96).msgs(msgs_per_item(msgs, msg_len, moff)), 8, st.data(), &d)) return 0;
    const size_t reached = (size_t)vmr_reach(st.data(), 0, n);              // the sets the reference's loop draws a scalar for
    if (reached) draw(user, rands.data(), (uint64_t)reached);
    if (reached < n) { vm_rng_drain(c); return 0; }                         // :273-275 (only the message phase is left to wait for)
    const int rc = vm_rng_phase2(c, g, rands.data(), false, d);
    std::fill(rands.begin(), rands.end(), 0);
    if (rc) { vm_rng_drain(c); return 0; }
    uint8_t r = 0;
    if (hipStreamSynchronize(c->hs_a) != hipSuccess) { vm_rng_drain(c); return 0; }
    c->ws_pending = false;
    if (g.dout.down(&r, 1) != hipSuccess) return 0;
    return r;
}

// ---- verify_multiple over a shared message list (include/mbls.h, mbls_verify_multiple*_shared_msgs): the entries above with the sets' messages named by index in
// a list that is hashed once. Grouped route: one Miller loop per message (the kernels of the k_vms_* family, mbls_vms.h); per-set route: every set gathers its point.
// The one way in for the device entries over a list or a resident table. d names its key handle alone (keys_in_table, keys_in_committees, keys_in_committee_span:
// the entry has seen the handles non-null); what the handle holds is read here, under the lock, where each entry's checks have always stood.
static int vm_shared_device(mbls_ctx* c, vm_call d, void* stream) {
    if (!c || !d.d_result) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    const uint64_t n = d.n; const int keys = vm_key_kind(d);
    if (d.mt && d.mt->c != c) ARGFAIL(c, "message table belongs to another context");
    if (d.locate && !d.d_set_results) ARGFAIL(c, "null set results");
    if (keys == VM_KEYS_SPAN) {
        const int rk = vm_keys_resolve(c, &d.ks, true); if (rk) return rk;
        if (n && (!d.ks.d_cmt_span_off || (d.ks.n_cmt_ids && !d.ks.d_cmt_ids) || (d.ks.bits_stride && !d.ks.d_bits))) ARGFAIL(c, "null key buffer");
    } else if (keys == VM_KEYS_COMMITTEE) {
        const int rk = vm_keys_resolve(c, &d.ks, true); if (rk) return rk;
        if (n && (!d.ks.d_cmt_idx || !d.ks.d_bits)) ARGFAIL(c, "null key buffer");
    } else {
        if (n && !(keys == VM_KEYS_TABLE ? (const void*)d.ks.d_idx : (const void*)d.d_apks)) ARGFAIL(c, "null key buffer");
        const int rk = vm_keys_resolve(c, &d.ks, true); if (rk) return rk;
    }
    if (n && !d.ms.d_idx) ARGFAIL(c, "null buffer");
    if (d.ms.n_msgs > 0xFFFFFFFFull || n > 0xFFFFFFFFull) ARGFAIL(c, "message indices and positions are 32-bit");
    return verify_multiple_impl(c, d, stream);
}
extern "C" int mbls_verify_multiple_shared_msgs_device(mbls_ctx* c, const uint8_t* d_sigs, const uint8_t* d_apks, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff,
        uint64_t n_msgs, const uint32_t* d_msg_idx, const uint64_t* d_rands, uint64_t n, uint8_t* d_result, uint32_t* d_status, void* stream) {
    return vm_shared_device(c, vm_sets(d_sigs, d_rands, n).keys_apks(d_apks).msgs(msgs_list(d_msgs, msg_len, d_moff, n_msgs, d_msg_idx)).out(d_result, d_status), stream);
}
extern "C" int mbls_verify_multiple_sets_indexed_shared_msgs_device(mbls_ctx* c, const mbls_keytable* t, const uint8_t* d_sigs, const uint32_t* d_key_idx, const uint32_t* d_offsets,
        uint32_t k, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff, uint64_t n_msgs, const uint32_t* d_msg_idx, const uint64_t* d_rands, uint64_t n,
        uint8_t* d_result, uint32_t* d_status, void* stream) {
    if (!t) return MBLS_ERR_ARGUMENT;
    return vm_shared_device(c, vm_sets(d_sigs, d_rands, n).keys(keys_in_table(t, d_key_idx, d_offsets), k).msgs(msgs_list(d_msgs, msg_len, d_moff, n_msgs, d_msg_idx))
                                   .out(d_result, d_status), stream);
}
// the host entries' checks (nothing is queued when they fail; the outputs stay untouched): the list's offset table, every index inside the list. -> the longest group
static int vm_shared_host_check(mbls_ctx* c, const vm_host& h, uint64_t* longest) {
    const uint64_t n_msgs = h.ms.n_msgs, n = h.n; const uint64_t* const moff = h.ms.d_moff; const uint32_t* const msg_idx = h.ms.d_idx;
    if (n_msgs > 0xFFFFFFFFull || n > 0xFFFFFFFFull) ARGFAIL(c, "message indices and positions are 32-bit");
    if (!h.sigs96 || !h.apks96 || !msg_idx) ARGFAIL(c, "null buffer");
    if (moff && !msg_offsets_ok(moff, n_msgs)) ARGFAIL(c, "msg_offsets must be non-decreasing, messages below 2^32 bytes");
    const size_t msg_total = moff ? (size_t)(moff[n_msgs] - moff[0]) : (size_t)h.ms.msg_len * n_msgs;
    if (!h.ms.d_msgs && msg_total) ARGFAIL(c, "null buffer");
    std::vector<uint32_t> cnt;
    try { cnt.assign(n_msgs, 0); } catch (...) { ARGFAIL(c, "out of host memory"); }
    uint64_t m = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (msg_idx[i] >= n_msgs) ARGFAIL(c, "msg_idx names no message of the list");
        if (++cnt[msg_idx[i]] > m) m = cnt[msg_idx[i]];
    }
    *longest = m;
    return MBLS_OK;
}
// the same for the host entries over a resident table (the caller holds the context's lock: the table's size is the one the call is planned with): every index
// names an entry of the table. -> the longest group and the number of distinct entries named, counted on a sorted copy of the indices (the table may be far
// larger than the call). The committee forms (h.hc) have no aggregate keys: apks96 is null
static int vm_msgtable_host_check(mbls_ctx* c, const vm_host& h, uint64_t* longest, uint64_t* named) {
    const uint64_t n = h.n; const uint32_t* const msg_idx = h.ms.d_idx;
    if (n > 0xFFFFFFFFull) ARGFAIL(c, "message indices and positions are 32-bit");
    if (!h.sigs96 || (!h.apks96 && !h.hc) || !msg_idx) ARGFAIL(c, "null buffer");
    for (uint64_t i = 0; i < n; i++)
        if (mtb_names_nothing(msg_idx[i], h.mt->size)) ARGFAIL(c, "msg_idx names no entry of the message table");
    std::vector<uint32_t> idx;
    try { idx.assign(msg_idx, msg_idx + n); } catch (...) { ARGFAIL(c, "out of host memory"); }
    std::sort(idx.begin(), idx.end());
    uint64_t m = 0, d = 0, run = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (i == 0 || idx[i] != idx[i - 1]) { d++; run = 0; }
        if (++run > m) m = run;
    }
    *longest = m; *named = d;
    return MBLS_OK;
}
// locate: the sets' answers as well (set_results required, set_status optional), staged behind one another in one buffer: n words, then n bytes
static int vm_shared_host_impl(mbls_ctx* c, const vm_host& h) {
    if (!c || !h.result) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    const uint64_t n = h.n, n_msgs = h.ms.n_msgs; const uint64_t* const moff = h.ms.d_moff;
    if (h.locate && !h.set_results) ARGFAIL(c, "null set results");
    if (n == 0) { *h.result = 1; if (h.status) *h.status = 0; return MBLS_OK; }
    if (!h.rands) ARGFAIL(c, "verify_multiple without blinding scalars is forgeable: rands must not be NULL");
    uint64_t longest = 0;
    int rc = vm_shared_host_check(c, h, &longest); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t msg_first = moff ? moff[0] : 0;
    const size_t msg_total = moff ? (size_t)(moff[n_msgs] - moff[0]) : (size_t)h.ms.msg_len * n_msgs;
    sbuf ds(c, 0), da(c, 1), dm(c, 2), dr(c, 3), dmo(c, 6), dres(c, 4), dmi(c, 7), dset(c, 8);
    HIPCHK(c, ds.up(h.sigs96, 96 * n)); HIPCHK(c, da.up(h.apks96, 96 * n)); HIPCHK(c, dm.up(h.ms.d_msgs ? h.ms.d_msgs + msg_first : nullptr, msg_total));
    HIPCHK(c, dr.up(h.rands, 8 * n)); HIPCHK(c, dmi.up(h.ms.d_idx, 4 * n)); HIPCHK(c, dres.alloc(8));
    if (moff) HIPCHK(c, dmo.up(moff, 8 * (n_msgs + 1)));
    uint32_t* d_sst = nullptr; uint8_t* d_sres = nullptr;
    if (h.locate) { HIPCHK(c, dset.alloc(5 * n)); d_sst = dset.as<uint32_t>(); d_sres = dset.as<uint8_t>() + 4 * n; }
    const vm_call d = vm_sets(ds.as<uint8_t>(), dr.as<uint64_t>(), n).keys_apks(da.as<uint8_t>())
                          .msgs(msgs_list(dm.as<uint8_t>() - msg_first, h.ms.msg_len, moff ? dmo.as<uint64_t>() : nullptr, n_msgs, dmi.as<uint32_t>()))
                          .out(dres.as<uint8_t>(), dres.as<uint32_t>() + 1).counted(longest);
    rc = vm_shared_device(c, h.locate ? d.out_sets(d_sres, d_sst) : d, c->hs_a);
    if (rc) { vm_rng_drain(c); return rc; }
    HIPCHK(c, hipStreamSynchronize(c->hs_a));
    c->ws_pending = false;
    uint32_t out[2] = {0, 0};
    HIPCHK(c, dres.down(out, 8));
    if (h.locate) {
        HIPCHK(c, hipMemcpy(h.set_results, d_sres, n, hipMemcpyDeviceToHost));
        if (h.set_status) HIPCHK(c, hipMemcpy(h.set_status, d_sst, 4 * n, hipMemcpyDeviceToHost));
    }
    *h.result = (uint8_t)(out[0] & 0xFF); if (h.status) *h.status = out[1];
    return MBLS_OK;
}
extern "C" int mbls_verify_multiple_shared_msgs(mbls_ctx* c, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs, uint32_t msg_len, const uint64_t* moff,
        uint64_t n_msgs, const uint32_t* msg_idx, const uint64_t* rands, uint64_t n, uint8_t* result, uint32_t* status) {
    return vm_shared_host_impl(c, vm_host_sets(sigs96, n).keys_apks(apks96).msgs(msgs_list(msgs, msg_len, moff, n_msgs, msg_idx)).scalars(rands).out(result, status));
}
// the reference's order, as mbls_verify_multiple_aggregate_signatures_rng keeps it (vm_rng_phase1 / vm_rng_phase2 with the list): signatures decoded and tested
// first, `draw` called once for the sets in front of the first bad signature, no second subgroup test
// locate: the sets' answers as well. A set at or behind the first signature outside G2 has no scalar (the reference never draws one) and cannot be examined: its
// answer is 0 and its word what the signature phase found, set on the host from the verdicts phase 1 read back (vmr_close). The sets in front of it have their
// scalars and are judged one by one: the call goes on (it is rejected through its status bits whatever the product is) with the scalar 1 for the sets without
// one, which changes nothing -- as mbls_verify_multiple_batches_locate_rng does.
// h.mt (the _msgtable entries): the sets' indices name entries of the resident table, no list; the host counts the named entries
// h.hc (the _committee_msgtable and _committee_span_msgtable entries, over h.mt): the sets' keys by descriptor word and bitfield (mbls_vmc.h) or by span
// (mbls_vcs.h) in host memory; a word or id that names nothing refuses the call
static int vm_shared_rng_impl(mbls_ctx* c, const vm_host& h) {
    if (!c || !h.result) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    const uint64_t n = h.n; const host_committees* const hc = h.hc;
    if (h.locate && !h.set_results) ARGFAIL(c, "null set results");
    if (h.mt && h.mt->c != c) ARGFAIL(c, "message table belongs to another context");
    vm_call d;
    if (hc) {
        d.ks = hc->span ? keys_in_committee_span(hc->t, nullptr, hc->n_cmt_ids, nullptr, nullptr, hc->bits_stride) : keys_in_committees(hc->t, nullptr, nullptr, hc->bits_stride);
        const int rk = vm_keys_resolve(c, &d.ks, false); if (rk) return rk;
    }
    if (n == 0) { *h.result = 1; return MBLS_OK; }                          // empty iterator: true, the generator untouched
    if (!h.draw) ARGFAIL(c, "no scalar source");
    if (hc && hc->span) { const int ri = vm_committee_span_sets_ok(c, *hc, d.ks, n); if (ri) return ri; }
    else if (hc) {
        if (!hc->cmt_idx || !hc->bits) ARGFAIL(c, "null buffer");
        for (uint64_t i = 0; i < n; i++)
            if (vmc_names_nothing(hc->cmt_idx[i], d.ks.ccount, d.ks.tsize))
                ARGFAIL(c, vmc_is_single(hc->cmt_idx[i]) ? "cmt_idx names no key of the key table" : "cmt_idx names no committee of the table");
    }
    d.mt = h.mt;
    int rc = h.mt ? vm_msgtable_host_check(c, h, &d.longest, &d.named) : vm_shared_host_check(c, h, &d.longest); if (rc) return rc;
    std::vector<uint64_t> rands; std::vector<uint32_t> st;
    try { rands.resize(n); st.resize(n); } catch (...) { ARGFAIL(c, "out of host memory"); }
    vm_rng_stage g(c);
    sbuf dset(c, 8);
    if (h.locate) {     // (the workspace of the WHOLE call, shadows included, is reserved by phase 1: growing it later would lose the decoded signatures)
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, dset.alloc(5 * n));
        d = d.out_sets(dset.as<uint8_t>() + 4 * n, dset.as<uint32_t>());
    }
    rc = vm_rng_phase1(c, g, h, 8, st.data(), &d); if (rc) return rc;
    const uint64_t reached = vmr_reach(st.data(), 0, n);                    // the sets the reference's loop draws a scalar for
    if (reached) h.draw(h.user, rands.data(), reached);
    if (reached < n && !h.locate) { vm_rng_drain(c); *h.result = 0; return MBLS_OK; }     // src/aggregates.rs:273-275
    for (uint64_t i = reached; i < n; i++) rands[i] = 1;
    rc = vm_rng_phase2(c, g, rands.data(), false, d);
    std::fill(rands.begin(), rands.end(), 0);
    if (rc) { vm_rng_drain(c); return rc; }
    if (hipStreamSynchronize(c->hs_a) != hipSuccess) { vm_rng_drain(c); return MBLS_ERR_DEVICE; }
    c->ws_pending = false;
    uint8_t r = 0;
    HIPCHK(c, g.dout.down(&r, 1));
    if (h.locate) {
        HIPCHK(c, hipMemcpy(h.set_results, d.d_set_results, n, hipMemcpyDeviceToHost));
        if (h.set_status) HIPCHK(c, hipMemcpy(h.set_status, d.d_set_status, 4 * n, hipMemcpyDeviceToHost));
        vmr_close(st.data(), &reached, nullptr, (uint32_t)n, 1, h.set_results, h.set_status);
    }
    *h.result = r;
    return MBLS_OK;
}
extern "C" int mbls_verify_multiple_shared_msgs_rng(mbls_ctx* c, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs, uint32_t msg_len, const uint64_t* moff,
        uint64_t n_msgs, const uint32_t* msg_idx, uint64_t n, uint8_t* result, mbls_scalar_source draw, void* user) {
    return vm_shared_rng_impl(c, vm_host_sets(sigs96, n).keys_apks(apks96).msgs(msgs_list(msgs, msg_len, moff, n_msgs, msg_idx)).source(draw, user).out(result, nullptr));
}
// ---- which sets of a rejected call over a shared message list (include/mbls.h, mbls_verify_multiple*_shared_msgs_locate*): the entries above with one bool and
// one status word per SET beside the call's own. Phase one is unchanged; the shadows, the mark rule and phase two are described at k_vsl_keep_key.
extern "C" int mbls_verify_multiple_shared_msgs_locate_device(mbls_ctx* c, const uint8_t* d_sigs, const uint8_t* d_apks, const uint8_t* d_msgs, uint32_t msg_len,
        const uint64_t* d_moff, uint64_t n_msgs, const uint32_t* d_msg_idx, const uint64_t* d_rands, uint64_t n, uint8_t* d_result, uint32_t* d_status,
        uint8_t* d_set_results, uint32_t* d_set_status, void* stream) {
    if (!d_set_results) return MBLS_ERR_ARGUMENT;
    return vm_shared_device(c, vm_sets(d_sigs, d_rands, n).keys_apks(d_apks).msgs(msgs_list(d_msgs, msg_len, d_moff, n_msgs, d_msg_idx)).out(d_result, d_status)
                                   .out_sets(d_set_results, d_set_status), stream);
}
extern "C" int mbls_verify_multiple_sets_indexed_shared_msgs_locate_device(mbls_ctx* c, const mbls_keytable* t, const uint8_t* d_sigs, const uint32_t* d_key_idx,
        const uint32_t* d_offsets, uint32_t k, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff, uint64_t n_msgs, const uint32_t* d_msg_idx,
        const uint64_t* d_rands, uint64_t n, uint8_t* d_result, uint32_t* d_status, uint8_t* d_set_results, uint32_t* d_set_status, void* stream) {
    if (!t || !d_set_results) return MBLS_ERR_ARGUMENT;
    return vm_shared_device(c, vm_sets(d_sigs, d_rands, n).keys(keys_in_table(t, d_key_idx, d_offsets), k).msgs(msgs_list(d_msgs, msg_len, d_moff, n_msgs, d_msg_idx))
                                   .out(d_result, d_status).out_sets(d_set_results, d_set_status), stream);
}
extern "C" int mbls_verify_multiple_shared_msgs_locate(mbls_ctx* c, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs, uint32_t msg_len, const uint64_t* moff,
        uint64_t n_msgs, const uint32_t* msg_idx, const uint64_t* rands, uint64_t n, uint8_t* result, uint32_t* status, uint8_t* set_results, uint32_t* set_status) {
    return vm_shared_host_impl(c, vm_host_sets(sigs96, n).keys_apks(apks96).msgs(msgs_list(msgs, msg_len, moff, n_msgs, msg_idx)).scalars(rands).out(result, status)
                                      .out_sets(set_results, set_status));
}
extern "C" int mbls_verify_multiple_shared_msgs_locate_rng(mbls_ctx* c, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs, uint32_t msg_len,
        const uint64_t* moff, uint64_t n_msgs, const uint32_t* msg_idx, uint64_t n, uint8_t* result, uint8_t* set_results, uint32_t* set_status, mbls_scalar_source draw,
        void* user) {
    return vm_shared_rng_impl(c, vm_host_sets(sigs96, n).keys_apks(apks96).msgs(msgs_list(msgs, msg_len, moff, n_msgs, msg_idx)).source(draw, user).out(result, nullptr)
                                     .out_sets(set_results, set_status));
}
// what a locate call over a shared list reserves before its first kernel: mbls_vsl.h's figure under the route and the list hash the limits choose
extern "C" uint64_t mbls_plan_verify_multiple_shared_msgs_locate_workspace_items(const mbls_limits* limits, uint64_t n, uint64_t n_msgs, int mode) {
    if (!limits || !n || mode < 0 || mode > 2) return 0;
    mbls_vm_shared_msgs_plan vp; plan_vm_shared(*limits, n, n_msgs, mode, 0, &vp);
    return vsl_workspace_items(n, n_msgs, vp.route == MBLS_VM_ROUTE_GROUPED, vp.list_workspace_items);
}

// ---- verify_multiple over the resident message table (include/mbls.h, mbls_verify_multiple*_msgtable*): the shared-message entries with a description that names
// a table in place of a list -- verify_multiple_impl's grouped route over the table's T entries, the named entries compacted on the device (mbls_vmt.h; k_vmt_flag,
// k_vmt_named, k_vmt_heads), or the per-set route with one gather from the table. Nothing is hashed.
extern "C" int mbls_verify_multiple_msgtable_device(mbls_ctx* c, const uint8_t* d_sigs, const uint8_t* d_apks, const mbls_msgtable* mt, const uint32_t* d_msg_idx,
        const uint64_t* d_rands, uint64_t n, uint8_t* d_result, uint32_t* d_status, void* stream) {
    if (!mt) return MBLS_ERR_ARGUMENT;
    return vm_shared_device(c, vm_sets(d_sigs, d_rands, n).keys_apks(d_apks).msgs_in(mt, d_msg_idx, 0).out(d_result, d_status), stream);
}
extern "C" int mbls_verify_multiple_sets_indexed_msgtable_device(mbls_ctx* c, const mbls_keytable* t, const uint8_t* d_sigs, const uint32_t* d_key_idx, const uint32_t* d_offsets,
        uint32_t k, const mbls_msgtable* mt, const uint32_t* d_msg_idx, const uint64_t* d_rands, uint64_t n, uint8_t* d_result, uint32_t* d_status, void* stream) {
    if (!t || !mt) return MBLS_ERR_ARGUMENT;
    return vm_shared_device(c, vm_sets(d_sigs, d_rands, n).keys(keys_in_table(t, d_key_idx, d_offsets), k).msgs_in(mt, d_msg_idx, 0).out(d_result, d_status), stream);
}
extern "C" int mbls_verify_multiple_msgtable_rng(mbls_ctx* c, const uint8_t* sigs96, const uint8_t* apks96, const mbls_msgtable* mt, const uint32_t* msg_idx, uint64_t n,
        uint8_t* result, mbls_scalar_source draw, void* user) {
    if (!mt) return MBLS_ERR_ARGUMENT;
    return vm_shared_rng_impl(c, vm_host_sets(sigs96, n).keys_apks(apks96).msgs_in(mt, msg_idx).source(draw, user).out(result, nullptr));
}
extern "C" int mbls_verify_multiple_msgtable_locate_device(mbls_ctx* c, const uint8_t* d_sigs, const uint8_t* d_apks, const mbls_msgtable* mt, const uint32_t* d_msg_idx,
        const uint64_t* d_rands, uint64_t n, uint8_t* d_result, uint32_t* d_status, uint8_t* d_set_results, uint32_t* d_set_status, void* stream) {
    if (!mt || !d_set_results) return MBLS_ERR_ARGUMENT;
    return vm_shared_device(c, vm_sets(d_sigs, d_rands, n).keys_apks(d_apks).msgs_in(mt, d_msg_idx, 0).out(d_result, d_status).out_sets(d_set_results, d_set_status), stream);
}
extern "C" int mbls_verify_multiple_sets_indexed_msgtable_locate_device(mbls_ctx* c, const mbls_keytable* t, const uint8_t* d_sigs, const uint32_t* d_key_idx,
        const uint32_t* d_offsets, uint32_t k, const mbls_msgtable* mt, const uint32_t* d_msg_idx, const uint64_t* d_rands, uint64_t n, uint8_t* d_result, uint32_t* d_status,
        uint8_t* d_set_results, uint32_t* d_set_status, void* stream) {
    if (!t || !mt || !d_set_results) return MBLS_ERR_ARGUMENT;
    return vm_shared_device(c, vm_sets(d_sigs, d_rands, n).keys(keys_in_table(t, d_key_idx, d_offsets), k).msgs_in(mt, d_msg_idx, 0).out(d_result, d_status)
                                   .out_sets(d_set_results, d_set_status), stream);
}
extern "C" int mbls_verify_multiple_msgtable_locate_rng(mbls_ctx* c, const uint8_t* sigs96, const uint8_t* apks96, const mbls_msgtable* mt, const uint32_t* msg_idx, uint64_t n,
        uint8_t* result, uint8_t* set_results, uint32_t* set_status, mbls_scalar_source draw, void* user) {
    if (!mt) return MBLS_ERR_ARGUMENT;
    return vm_shared_rng_impl(c, vm_host_sets(sigs96, n).keys_apks(apks96).msgs_in(mt, msg_idx).source(draw, user).out(result, nullptr).out_sets(set_results, set_status));
}

// ---- verify_multiple over committee bitfields and the resident message table (include/mbls.h, mbls_verify_multiple_committee_msgtable*; the set descriptor is
// mbls_vmc.h): the _sets_indexed_msgtable entries with every set's signers named by a committee id and its bitfield, or by one key index -- verify_multiple_impl's
// committee key source (k_vmc_expand, k_aggregate_vmc_d); everything behind the key sum is the entries' above.
extern "C" int mbls_verify_multiple_committee_msgtable_device(mbls_ctx* c, const mbls_committees* t, const uint8_t* d_sigs, const uint32_t* d_cmt_idx, const uint8_t* d_bits,
        uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* d_msg_idx, const uint64_t* d_rands, uint64_t n, uint8_t* d_result, uint32_t* d_status, void* stream) {
    if (!t || !mt) return MBLS_ERR_ARGUMENT;
    return vm_shared_device(c, vm_sets(d_sigs, d_rands, n).keys(keys_in_committees(t, d_cmt_idx, d_bits, bits_stride), 0).msgs_in(mt, d_msg_idx, 0).out(d_result, d_status), stream);
}
extern "C" int mbls_verify_multiple_committee_msgtable_locate_device(mbls_ctx* c, const mbls_committees* t, const uint8_t* d_sigs, const uint32_t* d_cmt_idx,
        const uint8_t* d_bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* d_msg_idx, const uint64_t* d_rands, uint64_t n, uint8_t* d_result,
        uint32_t* d_status, uint8_t* d_set_results, uint32_t* d_set_status, void* stream) {
    if (!t || !mt || !d_set_results) return MBLS_ERR_ARGUMENT;
    return vm_shared_device(c, vm_sets(d_sigs, d_rands, n).keys(keys_in_committees(t, d_cmt_idx, d_bits, bits_stride), 0).msgs_in(mt, d_msg_idx, 0).out(d_result, d_status)
                                   .out_sets(d_set_results, d_set_status), stream);
}
extern "C" int mbls_verify_multiple_committee_msgtable_rng(mbls_ctx* c, const mbls_committees* t, const uint8_t* sigs96, const uint32_t* cmt_idx, const uint8_t* bits,
        uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* msg_idx, uint64_t n, uint8_t* result, mbls_scalar_source draw, void* user) {
    if (!t || !mt) return MBLS_ERR_ARGUMENT;
    const host_committees hc = {t, cmt_idx, bits, bits_stride};
    return vm_shared_rng_impl(c, vm_host_sets(sigs96, n).keys(&hc).msgs_in(mt, msg_idx).source(draw, user).out(result, nullptr));
}
extern "C" int mbls_verify_multiple_committee_msgtable_locate_rng(mbls_ctx* c, const mbls_committees* t, const uint8_t* sigs96, const uint32_t* cmt_idx, const uint8_t* bits,
        uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* msg_idx, uint64_t n, uint8_t* result, uint8_t* set_results, uint32_t* set_status,
        mbls_scalar_source draw, void* user) {
    if (!t || !mt) return MBLS_ERR_ARGUMENT;
    const host_committees hc = {t, cmt_idx, bits, bits_stride};
    return vm_shared_rng_impl(c, vm_host_sets(sigs96, n).keys(&hc).msgs_in(mt, msg_idx).source(draw, user).out(result, nullptr).out_sets(set_results, set_status));
}

// ---- verify_multiple over committee spans and the resident message table (include/mbls.h, mbls_verify_multiple_committee_span_msgtable*; rules: mbls_vcs.h): the
// entries above with every set's signers named by a range of committee ids and one field over their concatenated members, or by one key index. The key source is
// verify_multiple_impl's committee source in its span form: k_vcs_expand, then k_aggregate_vcs_d or, under a split, k_vcs_partial_d and k_vcs_combine (mbls_vcs.hip).
extern "C" int mbls_verify_multiple_committee_span_msgtable_device(mbls_ctx* c, const mbls_committees* t, const uint8_t* d_sigs, const uint32_t* d_cmt_ids, uint64_t n_cmt_ids,
        const uint32_t* d_cmt_off, const uint8_t* d_bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* d_msg_idx, const uint64_t* d_rands, uint64_t n,
        uint8_t* d_result, uint32_t* d_status, void* stream) {
    if (!t || !mt) return MBLS_ERR_ARGUMENT;
    return vm_shared_device(c, vm_sets(d_sigs, d_rands, n).keys(keys_in_committee_span(t, d_cmt_ids, n_cmt_ids, d_cmt_off, d_bits, bits_stride), 0).msgs_in(mt, d_msg_idx, 0)
                                   .out(d_result, d_status), stream);
}
extern "C" int mbls_verify_multiple_committee_span_msgtable_locate_device(mbls_ctx* c, const mbls_committees* t, const uint8_t* d_sigs, const uint32_t* d_cmt_ids,
        uint64_t n_cmt_ids, const uint32_t* d_cmt_off, const uint8_t* d_bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* d_msg_idx, const uint64_t* d_rands,
        uint64_t n, uint8_t* d_result, uint32_t* d_status, uint8_t* d_set_results, uint32_t* d_set_status, void* stream) {
    if (!t || !mt || !d_set_results) return MBLS_ERR_ARGUMENT;
    return vm_shared_device(c, vm_sets(d_sigs, d_rands, n).keys(keys_in_committee_span(t, d_cmt_ids, n_cmt_ids, d_cmt_off, d_bits, bits_stride), 0).msgs_in(mt, d_msg_idx, 0)
                                   .out(d_result, d_status).out_sets(d_set_results, d_set_status), stream);
}
extern "C" int mbls_verify_multiple_committee_span_msgtable_rng(mbls_ctx* c, const mbls_committees* t, const uint8_t* sigs96, const uint32_t* cmt_ids, uint64_t n_cmt_ids,
        const uint32_t* cmt_off, const uint8_t* bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* msg_idx, uint64_t n, uint8_t* result,
        mbls_scalar_source draw, void* user) {
    if (!t || !mt) return MBLS_ERR_ARGUMENT;
    const host_committees hc = {t, nullptr, bits, bits_stride, true, cmt_ids, n_cmt_ids, cmt_off};
    return vm_shared_rng_impl(c, vm_host_sets(sigs96, n).keys(&hc).msgs_in(mt, msg_idx).source(draw, user).out(result, nullptr));
}
extern "C" int mbls_verify_multiple_committee_span_msgtable_locate_rng(mbls_ctx* c, const mbls_committees* t, const uint8_t* sigs96, const uint32_t* cmt_ids,
        uint64_t n_cmt_ids, const uint32_t* cmt_off, const uint8_t* bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* msg_idx, uint64_t n, uint8_t* result,
        uint8_t* set_results, uint32_t* set_status, mbls_scalar_source draw, void* user) {
    if (!t || !mt) return MBLS_ERR_ARGUMENT;
    const host_committees hc = {t, nullptr, bits, bits_stride, true, cmt_ids, n_cmt_ids, cmt_off};
    return vm_shared_rng_impl(c, vm_host_sets(sigs96, n).keys(&hc).msgs_in(mt, msg_idx).source(draw, user).out(result, nullptr).out_sets(set_results, set_status));
}

// ---- B independent verify_multiple batches in ONE call (include/mbls.h, mbls_verify_multiple_batches*): what B consecutive calls of the entries above return,
// one bool and one status word per batch. The per-set work (key sum, [r] apk, decode + subgroup test + [r] sig, message phase, one-pair Miller loop) is one lane
// per set and knows nothing of batches; what ties a batch together -- the sum of its blinded signatures, the product of its Miller values, its status word, its
// final exponentiation -- runs segmented: per-batch trees over the sets (k_g2_seg_tree_d, k_f12_seg_tree_d; rules in mbls_vmb.h), the B (S_b, -G1) pairs as
// workspace items [n, n + B) inside the sets' Miller launch, one final exponentiation per batch with verify_multiple's reject mask (k_vmb_final / k_vmb_final2).
// No value crosses a batch boundary. Routing by size with verify_multiple_impl's thresholds. Every fallible set-up step (reserve, staging, table_acquire) comes
// before the first kernel is enqueued on a side stream. Enqueues only.
// longest: the longest range of the table when the host has seen it (0: a device-side table -- any batch may hold every set, the trees get every level)
// sigs_resident / hash_enqueued: as in verify_multiple_impl (the _rng entry's second half)
// locate mode (mbls_verify_multiple_batches_locate*): phase one as without it, with the sets' blinded signatures and Miller values kept in shadow items before the
// trees run over them (k_vml_keep_sig, k_vml_keep_f), and phase two behind the per-batch tail: mark (k_vml_mark), then for the candidates -- the sets of rejected
// batches whose own word carries no rejecting bit -- the Miller loop of (sig, -G1), the product with f_i and a final exponentiation each. Enqueued whatever the
// verdicts are: the host never learns how many candidates there are, and waves without one return at once.
static int vmb_impl(mbls_ctx* c, const vm_call& d, void* stream) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    const uint64_t n = d.n, B = d.B; const uint32_t spb = d.spb; const uint32_t* const d_boff = d.d_boff; const uint64_t* const d_rands = d.d_rands;
    uint8_t* const d_results = d.d_result; uint32_t* const d_status = d.d_status_or; const bool loc = d.locate;
    uint64_t longest = d.longest;
    if (B == 0) { if (n) ARGFAIL(c, "sets without batches"); return MBLS_OK; }
    if (!d_results) ARGFAIL(c, "null results");
    if (loc && !d.d_set_results) ARGFAIL(c, "null set results");
    if (n > 0xFFFFFFFEull || B > 0xFFFFFFFEull) ARGFAIL(c, "set and batch indices are 32-bit");
    if (!d_boff && (uint64_t)spb * B != n) ARGFAIL(c, "n_sets != n_batches * sets_per_batch");
    if (n && !d_rands) ARGFAIL(c, "verify_multiple without blinding scalars is forgeable: rands must not be NULL");
    if (n && ((!d.d_sigs && !d.sigs_resident) || (!d.ms.d_msgs && d.ms.msg_len && !d.ms.d_moff))) ARGFAIL(c, "null buffer");
    if (n && !d.ks.indexed && !d.d_apks && !d.ks.d_pks) ARGFAIL(c, "null keys");
    if (n && d.ks.indexed && !d.ks.d_idx) ARGFAIL(c, "null key indices");
    keysrc ks = d.ks; const int keys = vm_key_kind(d);
    { const int rk = vm_keys_resolve(c, &ks, true); if (rk) return rk; }
    if (keys == VM_KEYS_WIRE && ks.fmt != MBLS_PK_COMPRESSED && ks.fmt != MBLS_PK_UNCOMPRESSED) ARGFAIL(c, "pk_format");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const bool pair_hash = n && n <= c->split_max_items && 2 * n <= c->round_items;       // as verify_multiple_impl decides
    const uint64_t sh = vml_shadow_first(n, B, pair_hash);         // locate mode: the first shadow item
    int rc = mbls_ctx_reserve(c, loc ? vml_workspace_items(n, B, pair_hash) : vmb_workspace_items(n, B, pair_hash)); if (rc) return rc;
    uint32_t* map = nullptr;
    sbuf dmap(c, 9);
    if (d_boff) { HIPCHK(c, dmap.alloc(4 * (n ? n : 1))); map = dmap.as<uint32_t>(); }
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    mbls_ws wv = ws; wv.w += n;                                    // the batches' view: item b of wv = workspace item n + b
    rc = ws_acquire(c, s); if (rc) return rc;
    if (keys == VM_KEYS_TABLE) { rc = table_acquire(c, ks.tab, s); if (rc) return rc; }
    uint32_t* st_set = c->d_status;                                // (cap >= n + 2 B words)
    uint32_t* st_batch = d_status ? d_status : c->d_status + n;
    uint32_t* owned = c->d_status + n + B;
    if (n && !d.sigs_resident) HIPCHK(c, hipMemsetAsync(st_set, 0, 4 * n, s));          // (resident: cleared before k_sig, and the message phase may be writing its bits)
    HIPCHK(c, hipMemsetAsync(c->d_status + n, 0, 8 * B, s));
    if (d_status) HIPCHK(c, hipMemsetAsync(d_status, 0, 4 * B, s));
    if (map) HIPCHK(c, hipMemsetAsync(map, 0xFF, 4 * (n ? n : 1), s));                // every entry the map kernel does not write reads as "no owner"
    HIPCHK(c, hipMemsetAsync(d_results, 0, B, s));                 // false until the tail kernel has spoken (fail closed)
    uint32_t* cand = c->d_status + vml_flags_first(n, B);          // (locate mode: cap >= 2 n + 2 B words)
    if (loc && n) {
        HIPCHK(c, hipMemsetAsync(d.d_set_results, 0, n, s));
        if (d.d_set_status) HIPCHK(c, hipMemsetAsync(d.d_set_status, 0, 4 * n, s));
        HIPCHK(c, hipMemsetAsync(cand, 0, 4 * n, s));
    }
    // the three chains side by side below half a round, as in verify_multiple_impl
    const bool fork = n && 2 * n <= c->round_items;
    hipStream_t s_sig = fork ? c->hs_b : s, s_msg = fork ? c->hs_c : s;
    if (fork) { HIPCHK(c, hipEventRecord(c->hs_ev, s)); HIPCHK(c, hipStreamWaitEvent(s_sig, c->hs_ev, 0)); HIPCHK(c, hipStreamWaitEvent(s_msg, c->hs_ev, 0)); }
    const bool hash_first = fork && !d.hash_enqueued;
    if (hash_first) launch_hash(c, ws, d.ms.d_msgs, d.ms.msg_len, d.ms.d_moff, st_set, n, s_msg, pair_hash);
    if (n) {
        if (keys == VM_KEYS_TABLE)
            hipLaunchKernelGGL(k_aggregate_indexed_d, dim3(nblk(n)), dim3(WG), 0, s, ws, ks.d_recs, ks.tsize, ks.d_idx, ks.d_off, d.k, MBLS_MODE_VERIFY, st_set, n);
        else if (keys == VM_KEYS_WIRE)
            launch_aggregate(ws, ks.d_pks, ks.d_off, d.k, ks.fmt, MBLS_MODE_VERIFY, st_set, n, s);
        hipLaunchKernelGGL(k_blind_g1_d, dim3(nblk(n)), dim3(WG), 0, s, ws, keys == VM_KEYS_APKS ? d.d_apks : (const uint8_t*)nullptr, d_rands, st_set, n);
        if (map) hipLaunchKernelGGL(k_vmb_set_map, dim3(nblk(B)), dim3(WG), 0, s_sig, d_boff, B, n, map);
        if (2 * n <= c->coop_max_items)      // small calls: the signature chain is what the call waits for -- two lanes per signature
            hipLaunchKernelGGL(k_blind_sig2_d, dim3(nblk(2 * n)), dim3(WG), 0, s_sig, ws, d.sigs_resident ? (const uint8_t*)nullptr : d.d_sigs, d_rands, st_set, n);
        else
            hipLaunchKernelGGL(k_blind_sig_d, dim3(nblk(n)), dim3(WG), 0, s_sig, ws, d.sigs_resident ? (const uint8_t*)nullptr : d.d_sigs, d_rands, st_set, n);
        if (!longest) longest = d_boff ? n : spb;
        if (loc) hipLaunchKernelGGL(k_vml_keep_sig, dim3(nblk(n)), dim3(WG), 0, s_sig, ws, n, sh);
        for (uint64_t half = 1; half < longest; half *= 2)         // S_b: the per-batch sums of the blinded signatures, left at the head of each range
            hipLaunchKernelGGL(k_g2_seg_tree_d, dim3(nblk(n)), dim3(WG), 0, s_sig, ws, (const uint32_t*)map, d_boff, spb, B, n, half);
        if (!(d.hash_enqueued && fork) && !hash_first) launch_hash(c, ws, d.ms.d_msgs, d.ms.msg_len, d.ms.d_moff, st_set, n, s_msg, pair_hash);
    }
    if (fork) {
        HIPCHK(c, hipEventRecord(c->hs_ev2, s_sig)); HIPCHK(c, hipEventRecord(c->hs_ev3, s_msg));
        HIPCHK(c, hipStreamWaitEvent(s, c->hs_ev2, 0)); HIPCHK(c, hipStreamWaitEvent(s, c->hs_ev3, 0));
    }
    // the B signature pairs join the sets: one Miller loop per workspace item [0, n + B) (set up only now: the lane-pair message phase works on items [0, 2 n))
    hipLaunchKernelGGL(k_vmb_sigpair_setup, dim3(nblk(B)), dim3(WG), 0, s, ws, d_boff, spb, B, n);
    if (2 * (n + B) <= c->coop_max_items)
        coop_run(c, COOP_MILLER1, ws, (uint64_t)0, (uint64_t)1, (uint64_t)0, n + B, (uint32_t*)nullptr, (uint8_t*)nullptr, COOP_RES_ITEM, s);
    else
        launch_miller_single(c, ws, n + B, s);
    if (n) {
        hipLaunchKernelGGL(k_vmb_status_fold, dim3(nblk(n)), dim3(WG), 0, s, (const uint32_t*)map, d_boff, spb, B, n, (const uint32_t*)st_set, st_batch, owned);
        if (loc) hipLaunchKernelGGL(k_vml_keep_f, dim3(nblk(n)), dim3(WG), 0, s, ws, n, sh);
        for (uint64_t half = 1; half < longest; half *= 2)         // the per-batch products of the sets' Miller values
            hipLaunchKernelGGL(k_f12_seg_tree_d, dim3(nblk(n)), dim3(WG), 0, s, ws, (const uint32_t*)map, d_boff, spb, B, n, half);
    }
    hipLaunchKernelGGL(k_vmb_gather, dim3(nblk(B)), dim3(WG), 0, s, ws, d_boff, spb, B, n, st_batch, (const uint32_t*)owned);
    hipLaunchKernelGGL(k_f12_tree_d, dim3(nblk(B)), dim3(WG), 0, s, wv, 2 * B, B);      // batch b <- (its signature pair) x (its sets' product)
    if (B <= c->split_max_items && 2 * B <= c->round_items) hipLaunchKernelGGL(k_vmb_final2, dim3(nblk(2 * B)), dim3(WG), 0, s, wv, st_batch, d_results, B);
    else hipLaunchKernelGGL(k_vmb_final, dim3(nblk(B)), dim3(WG), 0, s, wv, st_batch, d_results, B);
    if (loc && n) {
        hipLaunchKernelGGL(k_vml_mark, dim3(nblk(n)), dim3(WG), 0, s, ws, (const uint32_t*)map, d_boff, spb, B, n, (const uint32_t*)st_set, (const uint32_t*)owned,
                           (const uint8_t*)d_results, cand, d.d_set_results, d.d_set_status, sh);
        // the candidates' Miller loops over the shadow items, cut at rounds as launch_miller_single cuts: whole rounds, then the rest in the form its size allows
        const uint64_t R = c->round_items;
        const uint64_t full = n > R ? (n / R) * R : 0, rest = n - full;
        mbls_ws wsh = ws; wsh.w += sh;
        if (full) hipLaunchKernelGGL(k_vml_miller, dim3(nblk(full)), dim3(WG), 0, s, wsh, full, (const uint32_t*)cand);
        if (rest) {
            mbls_ws wr = wsh; wr.w += full;
            if (2 * rest <= R) hipLaunchKernelGGL(k_vml_miller2, dim3(nblk(2 * rest)), dim3(WG), 0, s, wr, rest, (const uint32_t*)(cand + full));
            else hipLaunchKernelGGL(k_vml_miller, dim3(nblk(rest)), dim3(WG), 0, s, wr, rest, (const uint32_t*)(cand + full));
        }
        hipLaunchKernelGGL(k_vml_product, dim3(nblk(n)), dim3(WG), 0, s, ws, n, sh, (const uint32_t*)cand);
        if (n <= c->split_max_items && 2 * n <= c->round_items)
            hipLaunchKernelGGL(k_vml_final2, dim3(nblk(2 * n)), dim3(WG), 0, s, ws, (const uint32_t*)st_set, (const uint32_t*)cand, d.d_set_results, d.d_set_status, n);
        else
            hipLaunchKernelGGL(k_vml_final, dim3(nblk(n)), dim3(WG), 0, s, ws, (const uint32_t*)st_set, (const uint32_t*)cand, d.d_set_results, d.d_set_status, n);
    }
    HIPCHK(c, hipGetLastError());
    return ws_release(c, s);
}
extern "C" int mbls_verify_multiple_batches_device(mbls_ctx* c, const uint8_t* d_sigs, const uint8_t* d_apks, const uint8_t* d_pks, int pk_format,
        const uint32_t* d_pk_offsets, uint32_t k, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff, const uint64_t* d_rands, uint64_t n,
        const uint32_t* d_batch_offsets, uint32_t sets_per_batch, uint64_t n_batches, uint8_t* d_results, uint32_t* d_status, void* stream) {
    const vm_call d = vm_sets(d_sigs, d_rands, n).msgs(msgs_per_item(d_msgs, msg_len, d_moff)).batches(d_batch_offsets, sets_per_batch, n_batches, 0).out(d_results, d_status);
    return vmb_impl(c, d_apks ? d.keys_apks(d_apks) : d.keys(keys_wire(d_pks, pk_format, d_pk_offsets), k), stream);
}
extern "C" int mbls_verify_multiple_batches_indexed_device(mbls_ctx* c, const mbls_keytable* t, const uint8_t* d_sigs, const uint32_t* d_key_idx, const uint32_t* d_offsets,
        uint32_t k, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff, const uint64_t* d_rands, uint64_t n, const uint32_t* d_batch_offsets,
        uint32_t sets_per_batch, uint64_t n_batches, uint8_t* d_results, uint32_t* d_status, void* stream) {
    if (!c || !t) return MBLS_ERR_ARGUMENT;
    return vmb_impl(c, vm_sets(d_sigs, d_rands, n).keys(keys_in_table(t, d_key_idx, d_offsets), k).msgs(msgs_per_item(d_msgs, msg_len, d_moff))
                           .batches(d_batch_offsets, sets_per_batch, n_batches, 0).out(d_results, d_status), stream);
}
extern "C" int mbls_verify_multiple_batches_locate_device(mbls_ctx* c, const uint8_t* d_sigs, const uint8_t* d_apks, const uint8_t* d_pks, int pk_format,
        const uint32_t* d_pk_offsets, uint32_t k, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff, const uint64_t* d_rands, uint64_t n,
        const uint32_t* d_batch_offsets, uint32_t sets_per_batch, uint64_t n_batches, uint8_t* d_results, uint32_t* d_status, uint8_t* d_set_results,
        uint32_t* d_set_status, void* stream) {
    const vm_call d = vm_sets(d_sigs, d_rands, n).msgs(msgs_per_item(d_msgs, msg_len, d_moff)).batches(d_batch_offsets, sets_per_batch, n_batches, 0).out(d_results, d_status)
                          .out_sets(d_set_results, d_set_status);
    return vmb_impl(c, d_apks ? d.keys_apks(d_apks) : d.keys(keys_wire(d_pks, pk_format, d_pk_offsets), k), stream);
}
extern "C" int mbls_verify_multiple_batches_locate_indexed_device(mbls_ctx* c, const mbls_keytable* t, const uint8_t* d_sigs, const uint32_t* d_key_idx,
        const uint32_t* d_offsets, uint32_t k, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff, const uint64_t* d_rands, uint64_t n,
        const uint32_t* d_batch_offsets, uint32_t sets_per_batch, uint64_t n_batches, uint8_t* d_results, uint32_t* d_status, uint8_t* d_set_results,
        uint32_t* d_set_status, void* stream) {
    if (!c || !t) return MBLS_ERR_ARGUMENT;
    return vmb_impl(c, vm_sets(d_sigs, d_rands, n).keys(keys_in_table(t, d_key_idx, d_offsets), k).msgs(msgs_per_item(d_msgs, msg_len, d_moff))
                           .batches(d_batch_offsets, sets_per_batch, n_batches, 0).out(d_results, d_status).out_sets(d_set_results, d_set_status), stream);
}
// what a locate call reserves before its first kernel (include/mbls.h): mbls_vml.h's figure under the limits' choice of the message phase
extern "C" uint64_t mbls_plan_locate_workspace_items(const mbls_limits* limits, uint64_t n_sets, uint64_t n_batches) {
    if (!limits || !n_batches) return 0;
    const bool pair_hash = n_sets && n_sets <= limits->split_max_items && 2 * n_sets <= limits->round_items;
    return vml_workspace_items(n_sets, n_batches, pair_hash);
}
// the host checks shared by the two host entries: the batch table (first 0, non-decreasing, last n) or the uniform count, the message table, the buffers
static int vmb_host_check(mbls_ctx* c, const vm_host& h, uint64_t* longest) {
    const uint64_t n = h.n, B = h.B; const uint32_t* const boff = h.boff; const uint64_t* const moff = h.ms.d_moff;
    if (!h.result) ARGFAIL(c, "null results");
    if (n > 0xFFFFFFFEull || B > 0xFFFFFFFEull) ARGFAIL(c, "set and batch indices are 32-bit");
    if (boff) { if (!vmb_offsets_ok(boff, B, n, longest)) ARGFAIL(c, "batch_offsets must start at 0, be non-decreasing and end at n_sets"); }
    else { if ((uint64_t)h.spb * B != n) ARGFAIL(c, "n_sets != n_batches * sets_per_batch"); *longest = h.spb; }
    if (moff && !msg_offsets_ok(moff, n)) ARGFAIL(c, "msg_offsets must be non-decreasing, messages below 2^32 bytes");
    const size_t msg_total = moff ? (size_t)(moff[n] - moff[0]) : (size_t)h.ms.msg_len * n;
    if (n && (!h.sigs96 || !h.apks96 || (!h.ms.d_msgs && msg_total))) ARGFAIL(c, "null buffer");
    return MBLS_OK;
}
// locate: the sets' answers as well (set_results required, set_status optional), staged behind one another in one buffer: n words, then n bytes
static int vmb_host_impl(mbls_ctx* c, const vm_host& h) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    const uint64_t n = h.n, B = h.B; const uint64_t* const moff = h.ms.d_moff;
    if (B == 0) { if (n) ARGFAIL(c, "sets without batches"); return MBLS_OK; }
    uint64_t longest = 0;
    int rc = vmb_host_check(c, h, &longest); if (rc) return rc;
    if (h.locate && !h.set_results) ARGFAIL(c, "null set results");
    if (n && !h.rands) ARGFAIL(c, "verify_multiple without blinding scalars is forgeable: rands must not be NULL");
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t msg_first = moff ? moff[0] : 0;
    const size_t msg_total = moff ? (size_t)(moff[n] - moff[0]) : (size_t)h.ms.msg_len * n;
    sbuf ds(c, 0), da(c, 1), dm(c, 2), dr(c, 3), dbo(c, 5), dmo(c, 6), dres(c, 7), dst(c, 8);
    HIPCHK(c, ds.up(h.sigs96, 96 * n)); HIPCHK(c, da.up(h.apks96, 96 * n)); HIPCHK(c, dm.up(h.ms.d_msgs ? h.ms.d_msgs + msg_first : nullptr, msg_total));
    HIPCHK(c, dr.up(h.rands, 8 * n));
    if (h.boff) HIPCHK(c, dbo.up(h.boff, 4 * (B + 1)));
    if (moff) HIPCHK(c, dmo.up(moff, 8 * (n + 1)));
    HIPCHK(c, dres.alloc(B)); HIPCHK(c, dst.alloc(4 * B));
    sbuf dset(c, 4);
    vm_call d = vm_sets(ds.as<uint8_t>(), dr.as<uint64_t>(), n).keys_apks(da.as<uint8_t>())
                    .msgs(msgs_per_item(dm.as<uint8_t>() - msg_first, h.ms.msg_len, moff ? dmo.as<uint64_t>() : nullptr))
                    .batches(h.boff ? dbo.as<uint32_t>() : nullptr, h.spb, B, 0).counted(longest ? longest : 1).out(dres.as<uint8_t>(), dst.as<uint32_t>());
    if (h.locate) { HIPCHK(c, dset.alloc(5 * n)); d = d.out_sets(dset.as<uint8_t>() + 4 * n, dset.as<uint32_t>()); }
    rc = vmb_impl(c, d, c->hs_a);
    if (rc) { vm_rng_drain(c); return rc; }
    HIPCHK(c, hipStreamSynchronize(c->hs_a));
    c->ws_pending = false;
    HIPCHK(c, dres.down(h.result, B));
    if (h.status) HIPCHK(c, dst.down(h.status, 4 * B));
    if (h.locate) {
        HIPCHK(c, hipMemcpy(h.set_results, d.d_set_results, n, hipMemcpyDeviceToHost));
        if (h.set_status) HIPCHK(c, hipMemcpy(h.set_status, d.d_set_status, 4 * n, hipMemcpyDeviceToHost));
    }
    return MBLS_OK;
}
extern "C" int mbls_verify_multiple_batches(mbls_ctx* c, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs, uint32_t msg_len, const uint64_t* moff,
        const uint64_t* rands, uint64_t n, const uint32_t* boff, uint32_t spb, uint64_t B, uint8_t* results, uint32_t* status) {
    return vmb_host_impl(c, vm_host_sets(sigs96, n).keys_apks(apks96).msgs(msgs_per_item(msgs, msg_len, moff)).scalars(rands).batches(boff, spb, B).out(results, status));
}
extern "C" int mbls_verify_multiple_batches_locate(mbls_ctx* c, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs, uint32_t msg_len, const uint64_t* moff,
        const uint64_t* rands, uint64_t n, const uint32_t* boff, uint32_t spb, uint64_t B, uint8_t* results, uint32_t* status, uint8_t* set_results,
        uint32_t* set_status) {
    return vmb_host_impl(c, vm_host_sets(sigs96, n).keys_apks(apks96).msgs(msgs_per_item(msgs, msg_len, moff)).scalars(rands).batches(boff, spb, B).out(results, status)
                                .out_sets(set_results, set_status));
}
// the second half of the batches' _rng entries, once the verdicts of the signature phase are in st: reach[b] for every batch, `draw` asked ONCE for exactly the
// scalars the reference's loops would have drawn (mbls_vmr.h), spread over the sets and uploaded to d_rands; the host copies are zeroed behind the upload
static int vmb_rng_scalars(mbls_ctx* c, const vm_host& h, const uint32_t* st, std::vector<uint64_t>& reach, sbuf& dr) {
    std::vector<uint64_t> rands, drawn;
    try { rands.resize(h.n); drawn.resize(h.n); reach.resize(h.B); } catch (...) { vm_rng_drain(c); ARGFAIL(c, "out of host memory"); }
    const uint64_t total = vmr_plan(st, h.boff, h.spb, h.B, reach.data());
    if (total) h.draw(h.user, drawn.data(), total);
    vmr_spread(drawn.data(), reach.data(), h.boff, h.spb, h.B, rands.data());
    const hipError_t e = dr.up(rands.data(), 8 * h.n);
    std::fill(rands.begin(), rands.end(), 0); std::fill(drawn.begin(), drawn.end(), 0);
    if (e != hipSuccess) { vm_rng_drain(c); return MBLS_ERR_DEVICE; }
    return MBLS_OK;
}
// ... and of their locate forms, once the call has run: the sets' answers come down, those at or behind their batch's reach are closed on the host (vmr_close)
static int vmb_rng_sets_down(mbls_ctx* c, const vm_host& h, const vm_call& d, const uint32_t* st, const std::vector<uint64_t>& reach) {
    std::vector<uint32_t> sst;
    try { sst.resize(h.n); } catch (...) { ARGFAIL(c, "out of host memory"); }
    HIPCHK(c, hipMemcpy(h.set_results, d.d_set_results, h.n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(sst.data(), d.d_set_status, 4 * h.n, hipMemcpyDeviceToHost));
    vmr_close(st, reach.data(), h.boff, h.spb, h.B, h.set_results, sst.data());
    if (h.set_status) memcpy(h.set_status, sst.data(), 4 * h.n);
    return MBLS_OK;
}
// The reference's order, generalised to B batches: B consecutive reference calls sharing one generator test batch b's signatures one by one and draw a scalar
// for every set in front of its first signature outside G2 (all of its sets when there is none), batch after batch (src/aggregates.rs:272-287). Here the
// signatures of ALL batches are decoded and tested first (vm_rng_phase1), the host reads the verdicts, `draw` is asked ONCE for exactly that sequence of
// scalars, and the rest runs without a second subgroup test (the points are in the slots). A batch with a bad signature is false through its status bits; its
// sets behind the bad one never had a scalar drawn and get the scalar 1, which changes nothing (the batch is rejected whatever its pairing product is).
// locate: the sets' answers as well. A set at or behind its batch's first signature outside G2 has no scalar (the reference never draws one): it cannot be
// examined -- its answer is 0 and its word what the signature phase found, set on the host from the verdicts phase 1 read back.
static int vmb_rng_impl(mbls_ctx* c, const vm_host& h) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    const uint64_t n = h.n, B = h.B;
    if (B == 0) { if (n) ARGFAIL(c, "sets without batches"); return MBLS_OK; }
    uint64_t longest = 0;
    int rc = vmb_host_check(c, h, &longest); if (rc) return rc;
    if (h.locate && !h.set_results) ARGFAIL(c, "null set results");
    if (n == 0) { memset(h.result, 1, B); return MBLS_OK; }                 // empty iterators: true, the generator untouched
    if (!h.draw) ARGFAIL(c, "null scalar source");
    std::vector<uint32_t> st; std::vector<uint64_t> reach;
    try { st.resize(n); } catch (...) { ARGFAIL(c, "out of host memory"); }
    HIPCHK(c, hipSetDevice(c->device));
    // everything that may allocate comes before the first kernel: the workspace of the WHOLE call (phase 1 alone would reserve less, and growing it later would
    // lose the decoded signatures), the staging of the table, the results and the map
    const bool pair_hash = n <= c->split_max_items && 2 * n <= c->round_items;
    rc = mbls_ctx_reserve(c, h.locate ? vml_workspace_items(n, B, pair_hash) : vmb_workspace_items(n, B, pair_hash)); if (rc) return rc;
    sbuf dbo(c, 5), dres(c, 7), dmap(c, 9), dset(c, 8);
    if (h.boff) { HIPCHK(c, dbo.up(h.boff, 4 * (B + 1))); HIPCHK(c, dmap.alloc(4 * n)); }
    HIPCHK(c, dres.alloc(B));
    vm_call d;
    if (h.locate) { HIPCHK(c, dset.alloc(5 * n)); d = d.out_sets(dset.as<uint8_t>() + 4 * n, dset.as<uint32_t>()); }
    vm_rng_stage g(c);
    rc = vm_rng_phase1(c, g, h, 8, st.data(), &d); if (rc) return rc;
    rc = vmb_rng_scalars(c, h, st.data(), reach, g.dr); if (rc) return rc;
    rc = vmb_impl(c, d.second_half(g.dr.as<uint64_t>(), true).batches(h.boff ? dbo.as<uint32_t>() : nullptr, h.spb, B, 0).counted(longest ? longest : 1)
                      .out(dres.as<uint8_t>(), nullptr), c->hs_a);
    if (rc) { vm_rng_drain(c); return rc; }
    if (hipStreamSynchronize(c->hs_a) != hipSuccess) { vm_rng_drain(c); return MBLS_ERR_DEVICE; }
    c->ws_pending = false;
    HIPCHK(c, dres.down(h.result, B));
    return h.locate ? vmb_rng_sets_down(c, h, d, st.data(), reach) : MBLS_OK;
}
extern "C" int mbls_verify_multiple_batches_rng(mbls_ctx* c, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs, uint32_t msg_len, const uint64_t* moff,
        uint64_t n, const uint32_t* boff, uint32_t spb, uint64_t B, uint8_t* results, mbls_scalar_source draw, void* user) {
    return vmb_rng_impl(c, vm_host_sets(sigs96, n).keys_apks(apks96).msgs(msgs_per_item(msgs, msg_len, moff)).source(draw, user).batches(boff, spb, B).out(results, nullptr));
}
extern "C" int mbls_verify_multiple_batches_locate_rng(mbls_ctx* c, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs, uint32_t msg_len,
        const uint64_t* moff, uint64_t n, const uint32_t* boff, uint32_t spb, uint64_t B, uint8_t* results, uint8_t* set_results, uint32_t* set_status,
        mbls_scalar_source draw, void* user) {
    return vmb_rng_impl(c, vm_host_sets(sigs96, n).keys_apks(apks96).msgs(msgs_per_item(msgs, msg_len, moff)).source(draw, user).batches(boff, spb, B).out(results, nullptr)
                               .out_sets(set_results, set_status));
}

// ---- B verify_multiple batches in one call over committee bitfields and the resident message table (include/mbls.h, mbls_verify_multiple_batches_committee_msgtable*;
// rules: mbls_vbg.h). The sets are the _committee_msgtable entries', the batches vmb_impl's, and every output is what vmb_impl writes for the spelled-out sets.
// PER-SET ROUTE: vmb_impl's chains with the key phase the committee source's (k_vmc_expand, k_aggregate_vmc_d) and the message phase the gather from the table.
// GROUPED ROUTE: one Miller loop per distinct (batch, entry) pair -- the kernels of mbls_vbg.hip. Workspace: the sets [0, n), over which the Miller items
// [0, B + bound) are laid once the blinded keys have moved to the positions [pbase, pbase + n); the tail's items [tail, tail + 2 B); for _locate the shadows
// A(i) = shf + i and B(i) = shf + n + i of mbls_vsl.h. The signature chain is vmb_impl's. Enqueues only; every fallible step comes before the first kernel on a
// side stream.
static void plan_vm_batches_committee(const mbls_limits& L, uint64_t n, uint64_t B, uint32_t spb, uint64_t T, uint64_t max_groups, int mode, bool locate,
                                      uint64_t longest_known, mbls_vm_batches_committee_plan* vp) {
    memset(vp, 0, sizeof(*vp));
    const uint64_t longest = vbg_longest(n, spb, longest_known), bound = vbg_bound(n, B, T, spb, max_groups, longest);
    const bool grouped = n && vbg_grouped(n, bound, mode);
    vp->route = grouped ? MBLS_VM_ROUTE_GROUPED : MBLS_VM_ROUTE_PER_SET;
    vp->bound = bound;
    vp->miller_items = vbg_miller_items(n, B, bound, grouped);
    vp->tree_levels = grouped ? vbg_key_levels(longest) : vmb_levels(longest);
    vp->product_levels = grouped ? vbg_product_levels(longest, bound) : vmb_levels(longest);
    vp->workspace_items = vbg_workspace_items(n, B, bound, grouped, locate);
    const uint64_t m = vp->miller_items, R = L.round_items;
    if (2 * m <= L.coop_max_items) vp->miller = MBLS_PAIRING_WAVE;
    else {
        const uint64_t full = (R && m > R) ? (m / R) * R : 0, rest = m - full;
        vp->miller = (rest && 2 * rest <= R) ? MBLS_PAIRING_LANES2 : MBLS_PAIRING_LANE;
    }
}
extern "C" int mbls_plan_verify_multiple_batches_committee(const mbls_limits* limits, uint64_t n_sets, uint64_t n_batches, uint32_t sets_per_batch, uint64_t table_size,
        uint64_t max_groups, int mode, int locate, mbls_vm_batches_committee_plan* out) {
    if (!limits || !out || !n_sets || !n_batches || mode < 0 || mode > 2) return MBLS_ERR_ARGUMENT;
    if (n_sets > 0xFFFFFFFEull || n_batches > 0xFFFFFFFEull || table_size > 0xFFFFFFFFull) return MBLS_ERR_ARGUMENT;
    if (sets_per_batch && (uint64_t)sets_per_batch * n_batches != n_sets) return MBLS_ERR_ARGUMENT;
    plan_vm_batches_committee(*limits, n_sets, n_batches, sets_per_batch, table_size, max_groups, mode, locate != 0, 0, out); return MBLS_OK;
}
// the span form (mbls_verify_multiple_batches_committee_span_msgtable*): the same plan; P = the split factor of the key phase on the call's n_sets (mbls_vcs.h
// vcs_split), whose partial sums stand behind the plan's items (mbls_vbg.h vbg_partial_first): workspace_items is raised by vcs_extra_items
extern "C" int mbls_plan_verify_multiple_batches_committee_span(const mbls_limits* limits, uint64_t n_sets, uint64_t n_batches, uint32_t sets_per_batch, uint64_t table_size,
        uint64_t max_groups, int mode, int locate, uint64_t stride_words, int split_mode, mbls_vm_batches_committee_plan* out, uint32_t* split) {
    if (!split || !vcs_split_mode_ok(split_mode)) return MBLS_ERR_ARGUMENT;
    const int rc = mbls_plan_verify_multiple_batches_committee(limits, n_sets, n_batches, sets_per_batch, table_size, max_groups, mode, locate, out); if (rc) return rc;
    const uint32_t P = vcs_split(n_sets, stride_words ? stride_words : 1, limits, split_mode);
    const bool grouped = out->route == MBLS_VM_ROUTE_GROUPED;
    out->workspace_items = vbg_partial_first(n_sets, n_batches, out->bound, grouped, locate != 0) + vcs_extra_items(n_sets, P);
    *split = P; return MBLS_OK;
}
static int vbg_impl(mbls_ctx* c, const vm_call& d, void* stream) {
    if (!c || !d.mt) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    const uint64_t n = d.n, B = d.B, max_groups = d.max_groups; const uint32_t spb = d.spb; const uint32_t* const d_boff = d.d_boff; const uint64_t* const d_rands = d.d_rands;
    const keysrc& ks = d.ks; const mbls_msgtable* const mt = d.mt; const uint32_t* const d_midx = d.ms.d_idx;
    uint8_t* const d_results = d.d_result; uint32_t* const d_status = d.d_status_or; const bool loc = d.locate;
    uint64_t longest = d.longest;
    if (B == 0) { if (n) ARGFAIL(c, "sets without batches"); return MBLS_OK; }
    if (!d_results) ARGFAIL(c, "null results");
    if (loc && !d.d_set_results) ARGFAIL(c, "null set results");
    if (n > 0xFFFFFFFEull || B > 0xFFFFFFFEull) ARGFAIL(c, "set and batch indices are 32-bit");
    if (!d_boff && (uint64_t)spb * B != n) ARGFAIL(c, "n_sets != n_batches * sets_per_batch");
    if (n && !d_rands) ARGFAIL(c, "verify_multiple without blinding scalars is forgeable: rands must not be NULL");
    const bool span = vm_key_kind(d) == VM_KEYS_SPAN;
    if (n && ((!d.d_sigs && !d.sigs_resident) || !d_midx)) ARGFAIL(c, "null buffer");
    if (n && (span ? !ks.d_cmt_span_off || (ks.n_cmt_ids && !ks.d_cmt_ids) || (ks.bits_stride && !ks.d_bits) : !ks.d_cmt_idx || !ks.d_bits)) ARGFAIL(c, "null buffer");
    if (mt->c != c) ARGFAIL(c, "message table belongs to another context");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const uint64_t T = mt->size;
    mbls_vm_batches_committee_plan vp;
    plan_vm_batches_committee(ctx_limits(c), n, B, d_boff ? 0u : spb, T, max_groups, c->vm_grouping, loc, longest, &vp);
    const bool grouped = vp.route == MBLS_VM_ROUTE_GROUPED;
    const uint64_t bound = vp.bound, n_miller = vp.miller_items;
    // the span form under a split: the partial sums' items behind everything the plan lays out (mbls_vbg.h vbg_partial_first); P = 1 for the committee form
    const uint32_t span_split = vm_committee_split(c, ks, n);
    int rc = mbls_ctx_reserve(c, vp.workspace_items + vcs_extra_items(n, span_split)); if (rc) return rc;
    if (n) { rc = span ? reserve_committee_span(c, n, keys_span_stride(ks)) : reserve_committee(c, n, ks.cmax); if (rc) return rc; }
    if (grouped) { rc = reserve_groups(c, vbg_group_words(n, B)); if (rc) return rc; }
    uint32_t* map = nullptr;
    sbuf dmap(c, 9);
    if (d_boff) { HIPCHK(c, dmap.alloc(4 * (n ? n : 1))); map = dmap.as<uint32_t>(); }
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    const uint64_t pbase = vbg_position_base(n, B, bound), tail = grouped ? vbg_tail_first(n, B, bound) : n;
    const uint64_t shf = grouped ? vbg_shadow_first(n, B, bound) : vml_shadow_first(n, B, false);     // locate mode: the first shadow item
    mbls_ws wv = ws; wv.w += tail;                                  // the batches' view: item b of wv = the batch's pair value, item B + b its sets' product
    rc = ws_acquire(c, s); if (rc) return rc;
    rc = msgtable_acquire(c, mt, s); if (rc) return rc;
    rc = committees_acquire(c, ks.cmt, s); if (rc) return rc;
    rc = table_acquire(c, ks.tab, s); if (rc) return rc;
    const uint32_t* const tab = mt->d_tab; const uint64_t tstride = mtb_stride(mt->cap); const uint32_t* const flags = mt->d_flag;
    uint32_t* st_set = c->d_status;                                 // (cap >= n + 2 B words; locate: 2 n + 2 B)
    uint32_t* st_batch = d_status ? d_status : c->d_status + n;
    uint32_t* owned = c->d_status + n + B;
    uint32_t* cand = c->d_status + vml_flags_first(n, B);
    mbls_vbg_arrays ga = {};
    if (grouped) {
        const uint64_t gc = c->hgrp_cap;
        ga.pos = c->d_hgrp; ga.rlo = c->d_hgrp + gc; ga.rhi = c->d_hgrp + 2 * gc; ga.head = c->d_hgrp + 3 * gc; ga.entry = c->d_hgrp + 4 * gc;
        ga.gcount = c->d_hgrp + 5 * gc; ga.goff = ga.gcount + B;   // (goff[0 .. B], then the live word: 2 B + 2 words)
    }
    uint32_t* const d_live = grouped ? ga.goff + B + 1 : nullptr;
    if (n && !d.sigs_resident) HIPCHK(c, hipMemsetAsync(st_set, 0, 4 * n, s));          // (resident: cleared before k_sig)
    HIPCHK(c, hipMemsetAsync(c->d_status + n, 0, 8 * B, s));
    if (d_status) HIPCHK(c, hipMemsetAsync(d_status, 0, 4 * B, s));
    if (map) HIPCHK(c, hipMemsetAsync(map, 0xFF, 4 * (n ? n : 1), s));
    HIPCHK(c, hipMemsetAsync(d_results, 0, B, s));                  // false until the tail kernel has spoken (fail closed)
    if (loc && n) {
        HIPCHK(c, hipMemsetAsync(d.d_set_results, 0, n, s));
        if (d.d_set_status) HIPCHK(c, hipMemsetAsync(d.d_set_status, 0, 4 * n, s));
        HIPCHK(c, hipMemsetAsync(cand, 0, 4 * n, s));
    }
    if (grouped) {
        HIPCHK(c, hipMemsetAsync(c->d_hgrp, 0xFF, 4 * 5 * c->hgrp_cap, s));      // positions, ranges, group records: none
        HIPCHK(c, hipMemsetAsync(ga.gcount, 0, 4 * (2 * B + 2), s));
    }
    // the map before the chains fork: the signatures' trees and the grouping both read it
    if (n && map) hipLaunchKernelGGL(k_vmb_set_map, dim3(nblk(B)), dim3(WG), 0, s, d_boff, B, n, map);
    const bool fork = n && 2 * n <= c->round_items;
    hipStream_t s_sig = fork ? c->hs_b : s, s_msg = fork ? c->hs_c : s;
    if (fork) { HIPCHK(c, hipEventRecord(c->hs_ev, s)); HIPCHK(c, hipStreamWaitEvent(s_sig, c->hs_ev, 0)); HIPCHK(c, hipStreamWaitEvent(s_msg, c->hs_ev, 0)); }
    if (!longest) longest = d_boff ? n : spb;
    if (n) {
        // the message phase of the per-set route: every set takes its entry's point (the grouped route reads the table from its Miller items)
        if (!grouped) hipLaunchKernelGGL(k_h_gather, dim3((unsigned)((n + MBLS_HB - 1) / MBLS_HB)), dim3(MBLS_HB), 0, s_msg, ws, tab, tstride, flags, d_midx, T, st_set, n);
        // the key phase: the committee source of verify_multiple_impl, or its span form
        if (span) vm_span_key_phase(c, ws, ks, n, span_split, vbg_partial_first(n, B, bound, grouped, loc), st_set, s);
        else {
            const uint64_t ls = keys_list_stride(ks);
            uint32_t* const cnt = c->d_cmt_cnt; uint32_t* const route = c->d_cmt_cnt + c->cmt_items;
            hipLaunchKernelGGL(k_vmc_expand, dim3((unsigned)n), dim3(WG), 0, s, ks.d_crecs, ks.ccount, ks.d_members, ks.d_cmt_idx, ks.d_bits, ks.bits_stride, c->cmt_route_mode,
                               c->d_cmt_list, ls, cnt, route, n);
            hipLaunchKernelGGL(k_aggregate_vmc_d, dim3(nblk(n)), dim3(WG), 0, s, ws, ks.d_recs, ks.tsize, (const uint32_t*)c->d_cmt_list, ls, (const uint32_t*)cnt, (const uint32_t*)route,
                               ks.d_crecs, ks.d_cmt_idx, st_set, n);
        }
        hipLaunchKernelGGL(k_blind_g1_d, dim3(nblk(n)), dim3(WG), 0, s, ws, (const uint8_t*)nullptr, d_rands, st_set, n);
        if (grouped) {      // groups, their offsets, the keys to their positions, the per-group sums: behind the keys on their stream
            mbls_vbg_launch_group(d_midx, T, d_boff, spb, B, n, (const uint32_t*)map, ga, st_set, s);
            hipLaunchKernelGGL(k_vms_scan, dim3(1), dim3(MBLS_VMS_SCAN_LANES), 0, s, (const uint32_t*)ga.gcount, B, ga.goff);
            if (loc) hipLaunchKernelGGL(k_vsl_keep_key, dim3(nblk(n)), dim3(WG), 0, s, ws, n, shf);      // [r_i] apk_i -> A(i), before the heads are written over the sets' items
            mbls_vbg_launch_scatter(ws, (const uint32_t*)ga.pos, n, pbase, s);
            mbls_ws wp = ws; wp.w += pbase;
            mbls_vbg_launch_key_trees(wp, (const uint32_t*)ga.rlo, (const uint32_t*)ga.rhi, n, vp.tree_levels, s);
        }
        if (2 * n <= c->coop_max_items)
            hipLaunchKernelGGL(k_blind_sig2_d, dim3(nblk(2 * n)), dim3(WG), 0, s_sig, ws, d.sigs_resident ? (const uint8_t*)nullptr : d.d_sigs, d_rands, st_set, n);
        else
            hipLaunchKernelGGL(k_blind_sig_d, dim3(nblk(n)), dim3(WG), 0, s_sig, ws, d.sigs_resident ? (const uint8_t*)nullptr : d.d_sigs, d_rands, st_set, n);
        if (loc) hipLaunchKernelGGL(k_vml_keep_sig, dim3(nblk(n)), dim3(WG), 0, s_sig, ws, n, grouped ? shf + n : shf);
        for (uint64_t half = 1; half < longest; half *= 2)         // S_b: the per-batch sums of the blinded signatures, left at the head of each range
            hipLaunchKernelGGL(k_g2_seg_tree_d, dim3(nblk(n)), dim3(WG), 0, s_sig, ws, (const uint32_t*)map, d_boff, spb, B, n, half);
    }
    if (fork) {
        HIPCHK(c, hipEventRecord(c->hs_ev2, s_sig)); HIPCHK(c, hipEventRecord(c->hs_ev3, s_msg));
        HIPCHK(c, hipStreamWaitEvent(s, c->hs_ev2, 0)); HIPCHK(c, hipStreamWaitEvent(s, c->hs_ev3, 0));
    }
    if (grouped) {
        if (n) hipLaunchKernelGGL(k_vmb_status_fold, dim3(nblk(n)), dim3(WG), 0, s, (const uint32_t*)map, d_boff, spb, B, n, (const uint32_t*)st_set, st_batch, owned);
        // (the heads leave the live Miller items, B + min(D, bound), in *d_live: waves above them return at once)
        mbls_vbg_launch_heads(ws, tab, tstride, flags, T, ga, d_boff, spb, B, n, bound, pbase, c->d_vmap, st_batch, d_live, s);
        if (2 * n_miller <= c->coop_max_items)
            coop_run(c, COOP_MILLER1, ws, (uint64_t)0, (uint64_t)1, (uint64_t)0, n_miller, (uint32_t*)nullptr, (uint8_t*)nullptr, COOP_RES_ITEM, s, (const uint32_t*)d_live);
        else
            launch_miller_single(c, ws, n_miller, s, (const uint32_t*)d_live);
        if (bound) {
            mbls_ws wg = ws; wg.w += B;                             // the group items' view
            uint64_t half = 1;
            for (uint32_t l = 0; l < vp.product_levels; l++, half *= 2)
                hipLaunchKernelGGL(k_f12_seg_tree_d, dim3(nblk(bound)), dim3(WG), 0, s, wg, (const uint32_t*)c->d_vmap, (const uint32_t*)ga.goff, 0u, B, bound, half);
        }
        mbls_vbg_launch_gather(ws, ga, d_boff, spb, B, n, bound, tail, st_batch, (const uint32_t*)owned, s);
    } else {
        // the B signature pairs join the sets: one Miller loop per workspace item [0, n + B)
        hipLaunchKernelGGL(k_vmb_sigpair_setup, dim3(nblk(B)), dim3(WG), 0, s, ws, d_boff, spb, B, n);
        if (2 * (n + B) <= c->coop_max_items)
            coop_run(c, COOP_MILLER1, ws, (uint64_t)0, (uint64_t)1, (uint64_t)0, n + B, (uint32_t*)nullptr, (uint8_t*)nullptr, COOP_RES_ITEM, s);
        else
            launch_miller_single(c, ws, n + B, s);
        if (n) {
            hipLaunchKernelGGL(k_vmb_status_fold, dim3(nblk(n)), dim3(WG), 0, s, (const uint32_t*)map, d_boff, spb, B, n, (const uint32_t*)st_set, st_batch, owned);
            if (loc) hipLaunchKernelGGL(k_vml_keep_f, dim3(nblk(n)), dim3(WG), 0, s, ws, n, shf);
            for (uint64_t half = 1; half < longest; half *= 2)     // the per-batch products of the sets' Miller values
                hipLaunchKernelGGL(k_f12_seg_tree_d, dim3(nblk(n)), dim3(WG), 0, s, ws, (const uint32_t*)map, d_boff, spb, B, n, half);
        }
        hipLaunchKernelGGL(k_vmb_gather, dim3(nblk(B)), dim3(WG), 0, s, ws, d_boff, spb, B, n, st_batch, (const uint32_t*)owned);
    }
    hipLaunchKernelGGL(k_f12_tree_d, dim3(nblk(B)), dim3(WG), 0, s, wv, 2 * B, B);      // batch b <- (its signature pair) x (its sets' product)
    if (B <= c->split_max_items && 2 * B <= c->round_items) hipLaunchKernelGGL(k_vmb_final2, dim3(nblk(2 * B)), dim3(WG), 0, s, wv, st_batch, d_results, B);
    else hipLaunchKernelGGL(k_vmb_final, dim3(nblk(B)), dim3(WG), 0, s, wv, st_batch, d_results, B);
    if (loc && n && grouped) {     // phase two of mbls_vsl.h with the set's batch in the place of the call: mark, both pairs' Miller loops, product, final
        mbls_ws wsa = ws; wsa.w += shf;
        mbls_vbg_launch_mark(wsa, tab, tstride, flags, d_midx, T, (const uint32_t*)map, d_boff, spb, B, n, (const uint32_t*)st_set, (const uint32_t*)owned,
                             (const uint8_t*)d_results, cand, d.d_set_results, d.d_set_status, s);
        vsl_examine(c, ws, n, shf, true, st_set, cand, d.d_set_results, d.d_set_status, s);
    } else if (loc && n) {         // vmb_impl's phase two
        hipLaunchKernelGGL(k_vml_mark, dim3(nblk(n)), dim3(WG), 0, s, ws, (const uint32_t*)map, d_boff, spb, B, n, (const uint32_t*)st_set, (const uint32_t*)owned,
                           (const uint8_t*)d_results, cand, d.d_set_results, d.d_set_status, shf);
        vsl_examine(c, ws, n, shf, false, st_set, cand, d.d_set_results, d.d_set_status, s);
    }
    HIPCHK(c, hipGetLastError());
    return ws_release(c, s);
}
// the device entries: the committee table read at the sizes it has now, then vbg_impl
static int vbg_device(mbls_ctx* c, vm_call d, void* stream) {
    if (!c || !d.ks.cmt || !d.mt) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (d.mt->c != c) ARGFAIL(c, "message table belongs to another context");
    const int rk = vm_keys_resolve(c, &d.ks, true); if (rk) return rk;
    return vbg_impl(c, d, stream);
}
extern "C" int mbls_verify_multiple_batches_committee_msgtable_device(mbls_ctx* c, const mbls_committees* t, const uint8_t* d_sigs, const uint32_t* d_cmt_idx,
        const uint8_t* d_bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* d_msg_idx, const uint64_t* d_rands, uint64_t n, const uint32_t* d_batch_offsets,
        uint32_t sets_per_batch, uint64_t n_batches, uint64_t max_groups, uint8_t* d_results, uint32_t* d_status, void* stream) {
    return vbg_device(c, vm_sets(d_sigs, d_rands, n).keys(keys_in_committees(t, d_cmt_idx, d_bits, bits_stride), 0).msgs_in(mt, d_msg_idx, 0)
                             .batches(d_batch_offsets, sets_per_batch, n_batches, max_groups).out(d_results, d_status), stream);
}
extern "C" int mbls_verify_multiple_batches_committee_msgtable_locate_device(mbls_ctx* c, const mbls_committees* t, const uint8_t* d_sigs, const uint32_t* d_cmt_idx,
        const uint8_t* d_bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* d_msg_idx, const uint64_t* d_rands, uint64_t n, const uint32_t* d_batch_offsets,
        uint32_t sets_per_batch, uint64_t n_batches, uint64_t max_groups, uint8_t* d_results, uint32_t* d_status, uint8_t* d_set_results, uint32_t* d_set_status,
        void* stream) {
    if (!d_set_results) return MBLS_ERR_ARGUMENT;
    return vbg_device(c, vm_sets(d_sigs, d_rands, n).keys(keys_in_committees(t, d_cmt_idx, d_bits, bits_stride), 0).msgs_in(mt, d_msg_idx, 0)
                             .batches(d_batch_offsets, sets_per_batch, n_batches, max_groups).out(d_results, d_status).out_sets(d_set_results, d_set_status), stream);
}
// the grow-only staging vbg_impl takes beside the workspace and the committee scratch, for calls of up to max_sets sets in up to max_batches batches: the set map
// of a ragged batch table and the group arrays of the grouped route. Not exported: a verify_multiple stream (mbls_stream.hip) reserves both at creation, so that
// no round of it allocates.
extern "C" __attribute__((visibility("hidden"))) int mblsi_vbg_reserve_staging(mbls_ctx* c, uint64_t max_sets, uint64_t max_batches) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    sbuf dmap(c, 9);
    HIPCHK(c, dmap.alloc(4 * (max_sets ? max_sets : 1)));
    return reserve_groups(c, vbg_group_words(max_sets, max_batches));
}
// host buffers, the draw order of vmb_rng_impl: the signatures of ALL batches are decoded and tested first, `draw` is asked once for the scalars of the sets in front
// of each batch's first signature outside G2, the rest runs without a second subgroup test. A committee id, key index or message index that names nothing, or a batch
// table that is not sound, refuses the call with nothing queued and the outputs untouched. The host counts the distinct (batch, entry) pairs itself.
static int vbg_rng_impl(mbls_ctx* c, const vm_host& h) {
    const host_committees* const hc = h.hc; const mbls_msgtable* const mt = h.mt;
    if (!c || !hc->t || !mt) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    const uint64_t n = h.n, B = h.B; const uint32_t spb = h.spb; const uint32_t* const boff = h.boff; const uint32_t* const msg_idx = h.ms.d_idx;
    if (mt->c != c) ARGFAIL(c, "message table belongs to another context");
    if (B == 0) { if (n) ARGFAIL(c, "sets without batches"); return MBLS_OK; }
    if (!h.result) ARGFAIL(c, "null results");
    if (h.locate && !h.set_results) ARGFAIL(c, "null set results");
    if (n > 0xFFFFFFFEull || B > 0xFFFFFFFEull) ARGFAIL(c, "set and batch indices are 32-bit");
    uint64_t longest = spb;
    if (boff) { if (!vmb_offsets_ok(boff, B, n, &longest)) ARGFAIL(c, "batch_offsets must start at 0, be non-decreasing and end at n_sets"); }
    else if ((uint64_t)spb * B != n) ARGFAIL(c, "n_sets != n_batches * sets_per_batch");
    keysrc ks = hc->span ? keys_in_committee_span(hc->t, nullptr, hc->n_cmt_ids, nullptr, nullptr, hc->bits_stride) : keys_in_committees(hc->t, nullptr, nullptr, hc->bits_stride);
    const int rk = vm_keys_resolve(c, &ks, false); if (rk) return rk;
    if (n == 0) { memset(h.result, 1, B); return MBLS_OK; }                 // empty iterators: true, the generator untouched
    if (!h.sigs96 || (!hc->span && (!hc->cmt_idx || !hc->bits)) || !msg_idx) ARGFAIL(c, "null buffer");
    if (!h.draw) ARGFAIL(c, "null scalar source");
    const uint64_t T = mt->size;
    if (hc->span) { const int ri = vm_committee_span_sets_ok(c, *hc, ks, n); if (ri) return ri; }
    for (uint64_t i = 0; i < n; i++) {
        if (!hc->span && vmc_names_nothing(hc->cmt_idx[i], ks.ccount, ks.tsize))
            ARGFAIL(c, vmc_is_single(hc->cmt_idx[i]) ? "cmt_idx names no key of the key table" : "cmt_idx names no committee of the table");
        if ((uint64_t)msg_idx[i] >= T) ARGFAIL(c, "msg_idx names no entry of the message table");
    }
    std::vector<uint64_t> reach; std::vector<uint32_t> st, seen;
    try { st.resize(n); } catch (...) { ARGFAIL(c, "out of host memory"); }
    // the distinct (batch, entry) pairs, counted the way the wave counts them: a set without an earlier set of its batch naming the same entry
    uint64_t groups = 0, lo, hi;
    for (uint64_t b = 0; b < B; b++) {
        vmr_batch_range(boff, spb, b, &lo, &hi);
        if (!vbg_batch_grouped(hi - lo)) { groups += hi - lo; continue; }
        try { seen.assign(msg_idx + lo, msg_idx + hi); } catch (...) { ARGFAIL(c, "out of host memory"); }
        std::sort(seen.begin(), seen.end());
        groups += (uint64_t)(std::unique(seen.begin(), seen.end()) - seen.begin());
    }
    HIPCHK(c, hipSetDevice(c->device));
    // everything that may allocate comes before the first kernel: the workspace of the WHOLE call, the committee scratch, the group arrays, the staging
    mbls_vm_batches_committee_plan vp;
    plan_vm_batches_committee(ctx_limits(c), n, B, boff ? 0u : spb, T, groups, c->vm_grouping, h.locate, longest, &vp);
    int rc = mbls_ctx_reserve(c, vp.workspace_items + vcs_extra_items(n, vm_committee_split(c, ks, n))); if (rc) return rc;      // (as vbg_impl will ask for it)
    rc = hc->span ? reserve_committee_span(c, n, keys_span_stride(ks)) : reserve_committee(c, n, ks.cmax); if (rc) return rc;
    if (vp.route == MBLS_VM_ROUTE_GROUPED) { rc = reserve_groups(c, vbg_group_words(n, B)); if (rc) return rc; }
    sbuf ds(c, 0), da(c, 1), dso(c, 2), dr(c, 3), dbo(c, 5), dres(c, 4), dmi(c, 7), dset(c, 8), dmap(c, 9), dci(c, 10);
    HIPCHK(c, ds.up(h.sigs96, 96 * n)); HIPCHK(c, da.up(hc->bits, (size_t)hc->bits_stride * n)); HIPCHK(c, dmi.up(msg_idx, 4 * n));
    HIPCHK(c, dr.alloc(8 * n)); HIPCHK(c, dres.alloc(B));
    if (boff) { HIPCHK(c, dbo.up(boff, 4 * (B + 1))); HIPCHK(c, dmap.alloc(4 * n)); }
    ks.d_bits = da.as<uint8_t>();
    if (hc->span) {     // the ids take the descriptor words' slot, the span offsets one of their own
        HIPCHK(c, dci.up(hc->cmt_ids, 4 * hc->n_cmt_ids)); HIPCHK(c, dso.up(hc->cmt_off, 4 * (n + 1)));
        ks.d_cmt_ids = dci.as<uint32_t>(); ks.d_cmt_span_off = dso.as<uint32_t>();
    } else { HIPCHK(c, dci.up(hc->cmt_idx, 4 * n)); ks.d_cmt_idx = dci.as<uint32_t>(); }
    vm_call d = vm_sets(nullptr, dr.as<uint64_t>(), n).keys(ks, 0).msgs_in(mt, dmi.as<uint32_t>(), 0).second_half(dr.as<uint64_t>(), false)
                    .batches(boff ? dbo.as<uint32_t>() : nullptr, spb, B, groups).counted(longest ? longest : 1).out(dres.as<uint8_t>(), nullptr);
    if (h.locate) { HIPCHK(c, dset.alloc(5 * n)); d = d.out_sets(dset.as<uint8_t>() + 4 * n, dset.as<uint32_t>()); }
    // the signatures: decoded and tested, the verdicts read back
    hipStream_t s = c->hs_a;
    mbls_ws ws; ws.w = c->d_w; ws.stride = c->cap;
    rc = ws_acquire(c, s); if (rc) return rc;
    if (vm_rng_signatures(c, ws, ds.as<uint8_t>(), n, s, false) || hipStreamSynchronize(s) != hipSuccess ||
        hipMemcpy(st.data(), c->d_status, 4 * n, hipMemcpyDeviceToHost) != hipSuccess) { vm_rng_drain(c); return MBLS_ERR_DEVICE; }
    rc = vmb_rng_scalars(c, h, st.data(), reach, dr); if (rc) return rc;
    rc = vbg_impl(c, d, s);
    if (rc) { vm_rng_drain(c); return rc; }
    if (hipStreamSynchronize(s) != hipSuccess) { vm_rng_drain(c); return MBLS_ERR_DEVICE; }
    c->ws_pending = false;
    HIPCHK(c, dres.down(h.result, B));
    return h.locate ? vmb_rng_sets_down(c, h, d, st.data(), reach) : MBLS_OK;
}
extern "C" int mbls_verify_multiple_batches_committee_msgtable_rng(mbls_ctx* c, const mbls_committees* t, const uint8_t* sigs96, const uint32_t* cmt_idx, const uint8_t* bits,
        uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* msg_idx, uint64_t n, const uint32_t* boff, uint32_t spb, uint64_t B, uint8_t* results,
        mbls_scalar_source draw, void* user) {
    const host_committees hc = {t, cmt_idx, bits, bits_stride};
    return vbg_rng_impl(c, vm_host_sets(sigs96, n).keys(&hc).msgs_in(mt, msg_idx).source(draw, user).batches(boff, spb, B).out(results, nullptr));
}
extern "C" int mbls_verify_multiple_batches_committee_msgtable_locate_rng(mbls_ctx* c, const mbls_committees* t, const uint8_t* sigs96, const uint32_t* cmt_idx,
        const uint8_t* bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* msg_idx, uint64_t n, const uint32_t* boff, uint32_t spb, uint64_t B,
        uint8_t* results, uint8_t* set_results, uint32_t* set_status, mbls_scalar_source draw, void* user) {
    const host_committees hc = {t, cmt_idx, bits, bits_stride};
    return vbg_rng_impl(c, vm_host_sets(sigs96, n).keys(&hc).msgs_in(mt, msg_idx).source(draw, user).batches(boff, spb, B).out(results, nullptr)
                               .out_sets(set_results, set_status));
}

// ---- B verify_multiple batches in one call over committee SPANS and the resident message table (include/mbls.h, mbls_verify_multiple_batches_committee_span_msgtable*):
// the entries above with the sets of mbls_verify_multiple_committee_span_msgtable* -- vbg_impl and vbg_rng_impl with the span form of the key source, whose key
// phase is verify_multiple_impl's (vm_span_key_phase). No kernel of its own.
extern "C" int mbls_verify_multiple_batches_committee_span_msgtable_device(mbls_ctx* c, const mbls_committees* t, const uint8_t* d_sigs, const uint32_t* d_cmt_ids,
        uint64_t n_cmt_ids, const uint32_t* d_cmt_off, const uint8_t* d_bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* d_msg_idx, const uint64_t* d_rands,
        uint64_t n, const uint32_t* d_batch_offsets, uint32_t sets_per_batch, uint64_t n_batches, uint64_t max_groups, uint8_t* d_results, uint32_t* d_status, void* stream) {
    return vbg_device(c, vm_sets(d_sigs, d_rands, n).keys(keys_in_committee_span(t, d_cmt_ids, n_cmt_ids, d_cmt_off, d_bits, bits_stride), 0).msgs_in(mt, d_msg_idx, 0)
                             .batches(d_batch_offsets, sets_per_batch, n_batches, max_groups).out(d_results, d_status), stream);
}
extern "C" int mbls_verify_multiple_batches_committee_span_msgtable_locate_device(mbls_ctx* c, const mbls_committees* t, const uint8_t* d_sigs, const uint32_t* d_cmt_ids,
        uint64_t n_cmt_ids, const uint32_t* d_cmt_off, const uint8_t* d_bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* d_msg_idx, const uint64_t* d_rands,
        uint64_t n, const uint32_t* d_batch_offsets, uint32_t sets_per_batch, uint64_t n_batches, uint64_t max_groups, uint8_t* d_results, uint32_t* d_status,
        uint8_t* d_set_results, uint32_t* d_set_status, void* stream) {
    if (!d_set_results) return MBLS_ERR_ARGUMENT;
    return vbg_device(c, vm_sets(d_sigs, d_rands, n).keys(keys_in_committee_span(t, d_cmt_ids, n_cmt_ids, d_cmt_off, d_bits, bits_stride), 0).msgs_in(mt, d_msg_idx, 0)
                             .batches(d_batch_offsets, sets_per_batch, n_batches, max_groups).out(d_results, d_status).out_sets(d_set_results, d_set_status), stream);
}
extern "C" int mbls_verify_multiple_batches_committee_span_msgtable_rng(mbls_ctx* c, const mbls_committees* t, const uint8_t* sigs96, const uint32_t* cmt_ids, uint64_t n_cmt_ids,
        const uint32_t* cmt_off, const uint8_t* bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* msg_idx, uint64_t n, const uint32_t* boff, uint32_t spb,
        uint64_t B, uint8_t* results, mbls_scalar_source draw, void* user) {
    const host_committees hc = {t, nullptr, bits, bits_stride, true, cmt_ids, n_cmt_ids, cmt_off};
    return vbg_rng_impl(c, vm_host_sets(sigs96, n).keys(&hc).msgs_in(mt, msg_idx).source(draw, user).batches(boff, spb, B).out(results, nullptr));
}
extern "C" int mbls_verify_multiple_batches_committee_span_msgtable_locate_rng(mbls_ctx* c, const mbls_committees* t, const uint8_t* sigs96, const uint32_t* cmt_ids,
        uint64_t n_cmt_ids, const uint32_t* cmt_off, const uint8_t* bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* msg_idx, uint64_t n, const uint32_t* boff,
        uint32_t spb, uint64_t B, uint8_t* results, uint8_t* set_results, uint32_t* set_status, mbls_scalar_source draw, void* user) {
    const host_committees hc = {t, nullptr, bits, bits_stride, true, cmt_ids, n_cmt_ids, cmt_off};
    return vbg_rng_impl(c, vm_host_sets(sigs96, n).keys(&hc).msgs_in(mt, msg_idx).source(draw, user).batches(boff, spb, B).out(results, nullptr)
                               .out_sets(set_results, set_status));
}
// test probe: steps 1-2 of the grouped route alone (k_vmb_set_map for a ragged table, k_vbg_group, k_vms_scan) on caller-given indices and batch table -- any
// table, faulty ones included -- with host buffers; every array over the sets has n_sets words, group_count n_batches, group_off n_batches + 1
extern "C" int mbls_vbg_group_probe(mbls_ctx* c, const uint32_t* msg_idx, uint64_t n, uint64_t table_size, const uint32_t* boff, uint32_t spb, uint64_t B,
        uint32_t* set_pos, uint32_t* set_status, uint32_t* pos_lo, uint32_t* pos_hi, uint32_t* group_head, uint32_t* group_entry, uint32_t* group_count,
        uint32_t* group_off) {
    if (!c) return MBLS_ERR_ARGUMENT;
    mbls_lock lk(c->mu);
    if (!B || (n && !msg_idx) || !set_pos || !set_status || !pos_lo || !pos_hi || !group_head || !group_entry || !group_count || !group_off) ARGFAIL(c, "null buffer");
    if (n > 0xFFFFFFFEull || B > 0xFFFFFFFEull || table_size > 0xFFFFFFFFull) ARGFAIL(c, "set and batch indices are 32-bit");
    if (!boff && (uint64_t)spb * B != n) ARGFAIL(c, "n_sets != n_batches * sets_per_batch");
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t nn = n ? n : 1;
    sbuf dmi(c, 7), dbo(c, 5), dmap(c, 9), darr(c, 8), dgc(c, 4);
    HIPCHK(c, dmi.up(msg_idx, 4 * n)); if (!n) HIPCHK(c, dmi.alloc(4));
    if (boff) { HIPCHK(c, dbo.up(boff, 4 * (B + 1))); HIPCHK(c, dmap.alloc(4 * nn)); }
    HIPCHK(c, darr.alloc(4 * 6 * nn)); HIPCHK(c, dgc.alloc(4 * (2 * B + 1)));
    hipStream_t s = c->hs_a;
    uint32_t* const a = darr.as<uint32_t>();
    mbls_vbg_arrays ga = {a, a + nn, a + 2 * nn, a + 3 * nn, a + 4 * nn, dgc.as<uint32_t>(), dgc.as<uint32_t>() + B};
    uint32_t* const st = a + 5 * nn;
    uint32_t* const map = boff ? dmap.as<uint32_t>() : nullptr;
    HIPCHK(c, hipMemsetAsync(a, 0xFF, 4 * 5 * nn, s)); HIPCHK(c, hipMemsetAsync(st, 0, 4 * nn, s)); HIPCHK(c, hipMemsetAsync(ga.gcount, 0, 4 * (2 * B + 1), s));
    if (map) {
        HIPCHK(c, hipMemsetAsync(map, 0xFF, 4 * nn, s));
        if (n) hipLaunchKernelGGL(k_vmb_set_map, dim3(nblk(B)), dim3(WG), 0, s, (const uint32_t*)dbo.as<uint32_t>(), B, n, map);
    }
    mbls_vbg_launch_group(dmi.as<uint32_t>(), table_size, boff ? (const uint32_t*)dbo.as<uint32_t>() : nullptr, spb, B, n, (const uint32_t*)map, ga, st, s);
    hipLaunchKernelGGL(k_vms_scan, dim3(1), dim3(MBLS_VMS_SCAN_LANES), 0, s, (const uint32_t*)ga.gcount, B, ga.goff);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    uint32_t* const outs[6] = {set_pos, pos_lo, pos_hi, group_head, group_entry, set_status};
    for (int u = 0; u < 6 && n; u++) HIPCHK(c, hipMemcpy(outs[u], a + (uint64_t)u * nn, 4 * n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(group_count, ga.gcount, 4 * B, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(group_off, ga.goff, 4 * (B + 1), hipMemcpyDeviceToHost));
    return MBLS_OK;
}

// ------------------------------------------------------------------------------------------------ several GPUs behind one handle
// items are independent (reference src/aggregates.rs:177-215 holds no state between calls), so a batch is cut
// into contiguous shards, one per device; each device has its own context, and one host thread per device stages and verifies its
// shard, writing results straight into the caller's buffers. No device talks to another. Key tables are replicated on every device.
#include <thread>
// RCCL, opened at run time: libmbls_hip.so has no link-time dependency on it (a host without RCCL, or a one-device handle that never exchanges anything, loads
// the library all the same). dlopen finds the copy the process already holds (PyTorch-ROCm ships its own librccl.so.1) before the one under /opt/rocm.
struct rccl_api {
    void* h = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
static bool rccl_open(rccl_api* a, char* why, size_t why_len) {
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* nm : names) { a->h = dlopen(nm, RTLD_NOW | RTLD_NOLOAD); if (a->h) break; }       // a copy the process holds already
    for (const char* nm : names) { if (a->h) break; a->h = dlopen(nm, RTLD_NOW | RTLD_LOCAL); }
    if (!a->h) { snprintf(why, why_len, "librccl.so.1 not found (%s)", dlerror()); return false; }
    a->CommInitAll = (decltype(a->CommInitAll))dlsym(a->h, "ncclCommInitAll");
    a->CommDestroy = (decltype(a->CommDestroy))dlsym(a->h, "ncclCommDestroy");
    a->GroupStart = (decltype(a->GroupStart))dlsym(a->h, "ncclGroupStart");
    a->GroupEnd = (decltype(a->GroupEnd))dlsym(a->h, "ncclGroupEnd");
    a->AllGather = (decltype(a->AllGather))dlsym(a->h, "ncclAllGather");
    a->GetErrorString = (decltype(a->GetErrorString))dlsym(a->h, "ncclGetErrorString");
    if (!a->CommInitAll || !a->CommDestroy || !a->GroupStart || !a->GroupEnd || !a->AllGather || !a->GetErrorString) {
        snprintf(why, why_len, "librccl.so.1 lacks an entry point"); return false;
    }
    return true;
}
// Several devices behind one handle. The exchange step of the paths that have one (the accept bitmap of mbls_multi_fast_aggregate_verify_bitmap, the partial
// records of mbls_multi_verify_multiple_aggregate_signatures) is an RCCL all-gather between the devices' buffers -- over xGMI on an MI355X node -- when the
// handle could set up a communicator; otherwise (RCCL absent, the same device listed twice: RCCL refuses duplicates, MBLS_MULTI_NO_RCCL set) the records travel
// through host memory and `rccl_note` says why. Never a restart, never a different result.
struct mbls_multi {
    std::vector<mbls_ctx*> ctx; char err[256] = {}; std::mutex mu;
    rccl_api rccl; std::vector<ncclComm_t> comms; bool rccl_on = false; char rccl_note[256] = {};
    std::vector<uint64_t*> d_bm_send, d_bm_all; uint64_t bm_words_cap = 0;        // per device: this shard's bitmap words / the gathered bitmap
    std::vector<uint8_t*> d_rec_all;                                              // per device: G partial records of verify_multiple
};
struct mbls_multi_keytable { mbls_multi* m = nullptr; std::vector<mbls_keytable*> tab; };

static void multi_rccl_setup(mbls_multi* m, const int* device_ids, int G) {
    if (getenv("MBLS_MULTI_NO_RCCL")) { snprintf(m->rccl_note, sizeof(m->rccl_note), "host join: MBLS_MULTI_NO_RCCL is set"); return; }
    for (int a = 0; a < G; a++) for (int b = a + 1; b < G; b++) if (device_ids[a] == device_ids[b]) {
        snprintf(m->rccl_note, sizeof(m->rccl_note), "host join: device %d is listed more than once (RCCL wants one rank per device)", device_ids[a]); return;
    }
    char why[160] = {};
    if (!rccl_open(&m->rccl, why, sizeof(why))) { snprintf(m->rccl_note, sizeof(m->rccl_note), "host join: %s", why); return; }
    m->comms.assign((size_t)G, nullptr);
    // RCCL may print a version banner to the C stdout when the first communicator of a process is made. The library does NOT touch the process-wide descriptor 1
    // for that by default (another thread of the host may be writing there in that window): an application that emits a protocol on stdout protects it itself, as
    // bench.py does (protect_stdout), or sets NCCL_DEBUG / RCCL's own switches. MBLS_MULTI_REDIRECT_STDOUT=1 opts a single-threaded host in to the old
    // behaviour: descriptor 1 points at stderr while the communicator is set up.
    const bool redirect = getenv("MBLS_MULTI_REDIRECT_STDOUT") != nullptr;
    int saved = -1;
    if (redirect) { fflush(stdout); saved = dup(1); if (saved >= 0) (void)dup2(2, 1); }
    const ncclResult_t r = m->rccl.CommInitAll(m->comms.data(), G, device_ids);
    if (redirect) { fflush(stdout); if (saved >= 0) { (void)dup2(saved, 1); (void)close(saved); } }
    if (r != ncclSuccess) {
        snprintf(m->rccl_note, sizeof(m->rccl_note), "host join: ncclCommInitAll failed: %s", m->rccl.GetErrorString(r)); m->comms.clear(); return;
    }
    m->rccl_on = true;
    snprintf(m->rccl_note, sizeof(m->rccl_note), "RCCL all-gather over a communicator of %d device(s)", G);
}
extern "C" int mbls_multi_create(mbls_multi** out, const int* device_ids, int n_devices) {
    if (!out || !device_ids || n_devices <= 0) return MBLS_ERR_ARGUMENT;
    mbls_multi* m = new (std::nothrow) mbls_multi();
    if (!m) return MBLS_ERR_DEVICE;
    for (int g = 0; g < n_devices; g++) {          // the same device may be listed more than once (two contexts share it)
        mbls_ctx* c = nullptr;
        int rc = mbls_ctx_create(&c, device_ids[g]);
        if (rc) { for (mbls_ctx* x : m->ctx) mbls_ctx_destroy(x); delete m; return rc; }
        m->ctx.push_back(c);
    }
    try {
        m->d_bm_send.assign((size_t)n_devices, nullptr); m->d_bm_all.assign((size_t)n_devices, nullptr); m->d_rec_all.assign((size_t)n_devices, nullptr);
        multi_rccl_setup(m, device_ids, n_devices);
    } catch (...) { for (mbls_ctx* x : m->ctx) mbls_ctx_destroy(x); delete m; return MBLS_ERR_DEVICE; }
    *out = m; return MBLS_OK;
}
extern "C" void mbls_multi_destroy(mbls_multi* m) {
    if (!m) return;
    for (size_t g = 0; g < m->ctx.size(); g++) {
        (void)hipSetDevice(m->ctx[g]->device); (void)hipDeviceSynchronize();
        if (g < m->comms.size() && m->comms[g]) (void)m->rccl.CommDestroy(m->comms[g]);
        if (m->d_bm_send[g]) (void)hipFree(m->d_bm_send[g]);
        if (m->d_bm_all[g]) (void)hipFree(m->d_bm_all[g]);
        if (m->d_rec_all[g]) (void)hipFree(m->d_rec_all[g]);
    }
    for (mbls_ctx* c : m->ctx) mbls_ctx_destroy(c);
    delete m;
}
// 1: the handle's exchange steps run as RCCL all-gathers between the devices; 0: through host memory (mbls_multi_exchange_note says why)
extern "C" int mbls_multi_rccl_active(const mbls_multi* m) { return m && m->rccl_on ? 1 : 0; }
extern "C" const char* mbls_multi_exchange_note(mbls_multi* m) { return m ? m->rccl_note : "null handle"; }
// Exchange `bytes` bytes per device: device g contributes d_send[g] and ends with all G contributions, in device order, in d_recv[g] (G * bytes). The devices'
// streams `st[g]` carry the operation; on return it has completed everywhere. RCCL when the handle has a communicator, host memory otherwise.
static int multi_allgather(mbls_multi* m, const std::vector<const void*>& d_send, const std::vector<void*>& d_recv, size_t bytes, const std::vector<hipStream_t>& st) {
    const size_t G = m->ctx.size();
    if (m->rccl_on) {
        ncclResult_t r = m->rccl.GroupStart();
        for (size_t g = 0; g < G && r == ncclSuccess; g++) {
            if (hipSetDevice(m->ctx[g]->device) != hipSuccess) { (void)m->rccl.GroupEnd(); snprintf(m->err, sizeof(m->err), "hipSetDevice failed"); return MBLS_ERR_DEVICE; }
            r = m->rccl.AllGather(d_send[g], d_recv[g], bytes, ncclUint8, m->comms[g], st[g]);
        }
        const ncclResult_t r2 = m->rccl.GroupEnd();
        if (r == ncclSuccess) r = r2;
        if (r != ncclSuccess) { snprintf(m->err, sizeof(m->err), "RCCL all-gather failed: %s", m->rccl.GetErrorString(r)); return MBLS_ERR_DEVICE; }
        for (size_t g = 0; g < G; g++) {
            if (hipSetDevice(m->ctx[g]->device) != hipSuccess || hipStreamSynchronize(st[g]) != hipSuccess) { snprintf(m->err, sizeof(m->err), "all-gather: device %d did not complete", m->ctx[g]->device); return MBLS_ERR_DEVICE; }
        }
        return MBLS_OK;
    }
    std::vector<uint8_t> host;
    try { host.resize(G * bytes); } catch (...) { snprintf(m->err, sizeof(m->err), "out of host memory"); return MBLS_ERR_DEVICE; }
    for (size_t g = 0; g < G; g++)
        if (hipSetDevice(m->ctx[g]->device) != hipSuccess || hipStreamSynchronize(st[g]) != hipSuccess ||
            hipMemcpy(host.data() + g * bytes, d_send[g], bytes, hipMemcpyDeviceToHost) != hipSuccess) { snprintf(m->err, sizeof(m->err), "host join: download from device %d failed", m->ctx[g]->device); return MBLS_ERR_DEVICE; }
    for (size_t g = 0; g < G; g++)
        if (hipSetDevice(m->ctx[g]->device) != hipSuccess || hipMemcpy(d_recv[g], host.data(), G * bytes, hipMemcpyHostToDevice) != hipSuccess) { snprintf(m->err, sizeof(m->err), "host join: upload to device %d failed", m->ctx[g]->device); return MBLS_ERR_DEVICE; }
    return MBLS_OK;
}
extern "C" int mbls_multi_device_count(const mbls_multi* m) { return m ? (int)m->ctx.size() : 0; }
extern "C" const char* mbls_multi_last_error(mbls_multi* m) { return m ? m->err : "null handle"; }
extern "C" mbls_ctx* mbls_multi_context(mbls_multi* m, int i) { return (m && i >= 0 && i < (int)m->ctx.size()) ? m->ctx[i] : nullptr; }
extern "C" int mbls_multi_reserve(mbls_multi* m, uint64_t max_items) {
    if (!m) return MBLS_ERR_ARGUMENT;
    const uint64_t G = m->ctx.size();
    for (mbls_ctx* c : m->ctx) { int rc = mbls_ctx_reserve(c, (max_items + G - 1) / G); if (rc) return rc; }
    return MBLS_OK;
}
// shard g of n items over G devices: [n g / G, n (g + 1) / G)  (the same partition as milagro_bls_amd/shard.py)
static inline uint64_t shard_lo(uint64_t n, uint64_t g, uint64_t G) { return (uint64_t)(((unsigned __int128)n * g) / G); }

static int multi_run(mbls_multi* m, const mbls_multi_keytable* mt, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len, const uint64_t* moff,
                     const uint8_t* pks, int fmt, const uint32_t* idx, const uint32_t* off, uint64_t n, uint32_t k, int mode, uint8_t* results, uint32_t* status) {
    if (!m || (mt && mt->m != m)) return MBLS_ERR_ARGUMENT;
    std::lock_guard<std::mutex> lk(m->mu);
    const uint64_t G = m->ctx.size();
    std::vector<int> rcs(G, MBLS_OK);
    std::vector<std::thread> th;
    // the call as a batch of HOST pointers: a shard is its slice
    const batch all{sigs, msgs_per_item(msgs, msg_len, moff), mt ? keys_table(nullptr, 0, idx, off, nullptr) : keys_wire(pks, fmt, off), n, k, mode, results, nullptr, status};
    auto work = [&](uint64_t g) {
        const uint64_t lo = shard_lo(n, g, G), hi = shard_lo(n, g + 1, G);
        if (hi == lo) return;
        const batch sh = slice(all, lo, hi);
        rcs[g] = verify_host(m->ctx[g], sh.d_sigs, sh.ms, nullptr, sh.ks.d_pks, fmt, mt ? mt->tab[g] : nullptr, sh.ks.d_idx, sh.ks.d_off, sh.n, k, mode, sh.d_results, sh.d_status);
    };
    try { for (uint64_t g = 1; g < G; g++) th.emplace_back(work, g); } catch (...) { for (auto& t : th) t.join(); snprintf(m->err, sizeof(m->err), "cannot start a host thread"); return MBLS_ERR_DEVICE; }
    work(0);
    for (auto& t : th) t.join();
    for (uint64_t g = 0; g < G; g++)
        if (rcs[g]) { snprintf(m->err, sizeof(m->err), "device %d (shard %llu): %s", m->ctx[g]->device, (unsigned long long)g, m->ctx[g]->err); return rcs[g]; }
    return MBLS_OK;
}
extern "C" int mbls_multi_fast_aggregate_verify_batch(mbls_multi* m, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len, const uint64_t* moff,
        const uint8_t* pks, int fmt, const uint32_t* off, uint64_t n, uint32_t k, uint8_t* results, uint32_t* status) {
    return multi_run(m, nullptr, sigs, msgs, msg_len, moff, pks, fmt, nullptr, off, n, k, MBLS_MODE_FAST_AGGREGATE, results, status);
}
extern "C" int mbls_multi_verify_batch(mbls_multi* m, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len, const uint64_t* moff, const uint8_t* pks, int fmt,
        uint64_t n, uint8_t* results, uint32_t* status) {
    return multi_run(m, nullptr, sigs, msgs, msg_len, moff, pks, fmt, nullptr, nullptr, n, 1, MBLS_MODE_VERIFY, results, status);
}
// verify_multiple over the devices of the handle: device g takes sets [n g / G, n (g + 1) / G) up to its partial record
// (one host thread per device), the records meet on the first device, which joins them and runs the tail. The same bool as the one-device call.
extern "C" int mbls_multi_verify_multiple_aggregate_signatures(mbls_multi* m, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs,
        uint32_t msg_len, const uint64_t* moff, const uint64_t* rands, size_t n) {
    if (!m) return 0;
    if (n == 0) return 1;
    if (moff && !msg_offsets_ok(moff, n)) return 0;
    if (!sigs96 || !apks96 || !rands || (!msgs && (moff ? moff[n] != moff[0] : msg_len != 0))) return 0;
    std::lock_guard<std::mutex> lk(m->mu);
    const uint64_t G = m->ctx.size();
    std::vector<int> rcs(G, MBLS_OK); std::vector<std::thread> th;
    std::vector<const void*> d_send(G, nullptr); std::vector<void*> d_recv(G, nullptr); std::vector<hipStream_t> st(G, nullptr);
    auto work = [&](uint64_t g) {
        mbls_ctx* c = m->ctx[g];
        const uint64_t lo = shard_lo(n, g, G), hi = shard_lo(n, g + 1, G), cnt = hi - lo;
        mbls_lock lk2(c->mu);
        if (hipSetDevice(c->device) != hipSuccess) { rcs[g] = MBLS_ERR_DEVICE; return; }
        if (!m->d_rec_all[g] && hipMalloc(&m->d_rec_all[g], G * MBLS_VM_PARTIAL_BYTES) != hipSuccess) { m->d_rec_all[g] = nullptr; rcs[g] = MBLS_ERR_DEVICE; return; }
        const uint64_t first = moff ? moff[lo] : (uint64_t)msg_len * lo;
        const size_t mbytes = moff ? (size_t)(moff[hi] - moff[lo]) : (size_t)msg_len * cnt;
        sbuf ds(c, 0), da(c, 1), dm(c, 2), dr(c, 3), dmo(c, 6), drec(c, 4);
        if (ds.up(sigs96 + 96 * lo, 96 * cnt) != hipSuccess || da.up(apks96 + 96 * lo, 96 * cnt) != hipSuccess ||
            dm.up(msgs ? msgs + first : nullptr, mbytes) != hipSuccess || dr.up(rands + lo, 8 * cnt) != hipSuccess ||
            (moff && dmo.up(moff + lo, 8 * (cnt + 1)) != hipSuccess) || drec.alloc(MBLS_VM_PARTIAL_BYTES) != hipSuccess) { rcs[g] = MBLS_ERR_DEVICE; return; }
        // offset tables are absolute: the staged message bytes start at the shard's first offset
        rcs[g] = mbls_verify_multiple_partial_device(c, ds.as<uint8_t>(), da.as<uint8_t>(), nullptr, 0, nullptr, 0, dm.as<uint8_t>() - (moff ? first : 0), msg_len,
                                                     moff ? dmo.as<uint64_t>() : nullptr, dr.as<uint64_t>(), cnt, drec.as<uint8_t>(), c->hs_a);
        const bool synced = hipStreamSynchronize(c->hs_a) == hipSuccess;
        (void)hipStreamSynchronize(c->hs_b); (void)hipStreamSynchronize(c->hs_c);
        c->ws_pending = false;
        if (!rcs[g] && !synced) rcs[g] = MBLS_ERR_DEVICE;
        d_send[g] = drec.p; d_recv[g] = m->d_rec_all[g]; st[g] = c->hs_a;       // the shard's record stays on its device: the exchange step follows
    };
    try { for (uint64_t g = 1; g < G; g++) th.emplace_back(work, g); } catch (...) { for (auto& t : th) t.join(); snprintf(m->err, sizeof(m->err), "cannot start a host thread"); return 0; }
    work(0);
    for (auto& t : th) t.join();
    for (uint64_t g = 0; g < G; g++)
        if (rcs[g]) { snprintf(m->err, sizeof(m->err), "device %d (shard %llu): %s", m->ctx[g]->device, (unsigned long long)g, m->ctx[g]->err); return 0; }
    // THE exchange step: every device ends with all G records -- an RCCL all-gather of G x 896 bytes between the devices when the handle
    // has a communicator, host memory otherwise; the join then runs on the first device (any of them would reach the same bool)
    if (multi_allgather(m, d_send, d_recv, MBLS_VM_PARTIAL_BYTES, st)) return 0;
    mbls_ctx* c = m->ctx[0];
    mbls_lock lk0(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return 0;
    sbuf dres(c, 4); uint8_t r = 0;
    if (dres.alloc(8) != hipSuccess) return 0;
    if (mbls_verify_multiple_finish_device(c, m->d_rec_all[0], G, dres.as<uint8_t>(), nullptr, c->hs_a)) { (void)hipStreamSynchronize(c->hs_a); c->ws_pending = false; return 0; }
    if (hipStreamSynchronize(c->hs_a) != hipSuccess) return 0;
    c->ws_pending = false;
    if (dres.down(&r, 1) != hipSuccess) return 0;
    return r;
}
// The same over several devices with the reference's RNG ORDER and without a second subgroup test (what mbls_verify_multiple_aggregate_signatures_rng is to one
// device): every device decodes and tests its shard's signatures (they stay in its workspace) beside its message phase; the host reads the verdicts, finds the first
// bad signature of the WHOLE batch, asks `draw` once for the scalars of the sets in front of it (reference src/aggregates.rs:272-287), and -- all signatures good --
// every device goes on to its record, the records are exchanged (RCCL / host) and joined. One host thread per device holds its context across both phases.
#include <condition_variable>
extern "C" int mbls_multi_verify_multiple_aggregate_signatures_rng(mbls_multi* m, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs,
        uint32_t msg_len, const uint64_t* moff, size_t n, mbls_scalar_source draw, void* user) {
    if (!m) return 0;
    if (n == 0) return 1;                                                   // empty iterator: true, the generator untouched
    if (!draw) return 0;
    if (moff && !msg_offsets_ok(moff, n)) return 0;
    if (!sigs96 || !apks96 || (!msgs && (moff ? moff[n] != moff[0] : msg_len != 0))) return 0;
    std::lock_guard<std::mutex> lk(m->mu);
    const uint64_t G = m->ctx.size();
    std::vector<uint64_t> rands; std::vector<uint32_t> stw;
    try { rands.resize(n); stw.resize(n); } catch (...) { return 0; }
    std::vector<int> rcs(G, MBLS_OK); std::vector<std::thread> th;
    std::vector<const void*> d_send(G, nullptr); std::vector<void*> d_recv(G, nullptr); std::vector<hipStream_t> st(G, nullptr);
    std::mutex bm; std::condition_variable cv; uint64_t arrived = 0; int go = 0;             // go: 1 = run phase 2, -1 = stop (a bad signature, or a failed shard)
    auto work = [&](uint64_t g) {
        mbls_ctx* c = m->ctx[g];
        const uint64_t lo = shard_lo(n, g, G), hi = shard_lo(n, g + 1, G), cnt = hi - lo;
        mbls_lock lk2(c->mu);
        vm_rng_stage sg(c);
        if (hipSetDevice(c->device) != hipSuccess) rcs[g] = MBLS_ERR_DEVICE;
        if (!rcs[g] && !m->d_rec_all[g] && hipMalloc(&m->d_rec_all[g], G * MBLS_VM_PARTIAL_BYTES) != hipSuccess) { m->d_rec_all[g] = nullptr; rcs[g] = MBLS_ERR_DEVICE; }
        // (offset tables are absolute: phase 1 stages the shard's message bytes from its first offset on)
        vm_call d;
        if (!rcs[g]) rcs[g] = vm_rng_phase1(c, sg, vm_host_sets(sigs96 + 96 * lo, cnt).keys_apks(apks96 + 96 * lo)
                                                .msgs(msgs_per_item(moff ? msgs : (msgs ? msgs + (uint64_t)msg_len * lo : nullptr), msg_len, moff ? moff + lo : nullptr)),
                                            MBLS_VM_PARTIAL_BYTES, stw.data() + lo, &d);
        int mine;
        {
            std::unique_lock<std::mutex> ul(bm);
            arrived++; cv.notify_all();
            cv.wait(ul, [&] { return go != 0; });
            mine = go;
        }
        if (mine < 0 || rcs[g]) { if (cnt) vm_rng_drain(c); return; }
        rcs[g] = vm_rng_phase2(c, sg, rands.data() + lo, true, d);
        const bool synced = hipStreamSynchronize(c->hs_a) == hipSuccess;
        (void)hipStreamSynchronize(c->hs_b); (void)hipStreamSynchronize(c->hs_c);
        c->ws_pending = false;
        if (!rcs[g] && !synced) rcs[g] = MBLS_ERR_DEVICE;
        d_send[g] = sg.dout.p; d_recv[g] = m->d_rec_all[g]; st[g] = c->hs_a;       // the shard's record stays on its device: the exchange step follows
    };
    try { for (uint64_t g = 0; g < G; g++) th.emplace_back(work, g); }
    catch (...) {
        { std::lock_guard<std::mutex> gl(bm); go = -1; } cv.notify_all();
        for (auto& t : th) t.join();
        snprintf(m->err, sizeof(m->err), "cannot start a host thread"); return 0;
    }
    bool proceed = true;
    {
        std::unique_lock<std::mutex> ul(bm);
        cv.wait(ul, [&] { return arrived == G; });
    }
    for (uint64_t g = 0; g < G; g++) if (rcs[g]) proceed = false;
    if (proceed) {
        const size_t reached = (size_t)vmr_reach(stw.data(), 0, n);
        if (reached) draw(user, rands.data(), (uint64_t)reached);
        if (reached < n) proceed = false;                                   // :273-275
    }
    { std::lock_guard<std::mutex> gl(bm); go = proceed ? 1 : -1; } cv.notify_all();
    for (auto& t : th) t.join();
    std::fill(rands.begin(), rands.end(), 0);
    for (uint64_t g = 0; g < G; g++)
        if (rcs[g]) { snprintf(m->err, sizeof(m->err), "device %d (shard %llu): %s", m->ctx[g]->device, (unsigned long long)g, m->ctx[g]->err); return 0; }
    if (!proceed) return 0;
    if (multi_allgather(m, d_send, d_recv, MBLS_VM_PARTIAL_BYTES, st)) return 0;
    mbls_ctx* c = m->ctx[0];
    mbls_lock lk0(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return 0;
    sbuf dres(c, 5); uint8_t r = 0;
    if (dres.alloc(8) != hipSuccess) return 0;
    if (mbls_verify_multiple_finish_device(c, m->d_rec_all[0], G, dres.as<uint8_t>(), nullptr, c->hs_a)) { (void)hipStreamSynchronize(c->hs_a); c->ws_pending = false; return 0; }
    if (hipStreamSynchronize(c->hs_a) != hipSuccess) return 0;
    c->ws_pending = false;
    if (dres.down(&r, 1) != hipSuccess) return 0;
    return r;
}
// n x fast_aggregate_verify over the handle's devices with the results as ONE packed accept bitmap that every device ends up holding (north_star: "RCCL over
// xGMI used only to gather the final accept bitmap"): device g verifies the items of bitmap words [g W, (g + 1) W), W = ceil(ceil(n / 64) / G), packs its W words
// on the device, and the words are all-gathered between the devices (multi_allgather). `bitmap` (host, ceil(n / 64) words, optional) receives device 0's copy;
// mbls_multi_device_bitmap(m, g) is device g's copy (G W words, valid until the next call on the handle). Host buffers in, like the other handle entries.
extern "C" int mbls_multi_fast_aggregate_verify_bitmap(mbls_multi* m, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len, const uint64_t* moff,
        const uint8_t* pks, int fmt, const uint32_t* off, uint64_t n, uint32_t k, uint64_t* bitmap, uint32_t* status) {
    if (!m) return MBLS_ERR_ARGUMENT;
    if (n == 0) return MBLS_OK;
    std::lock_guard<std::mutex> lk(m->mu);
    const uint64_t G = m->ctx.size();
    const uint64_t words = (n + 63) / 64, W = (words + G - 1) / G;
    const batch all{sigs, msgs_per_item(msgs, msg_len, moff), keys_wire(pks, fmt, off), n, k, MBLS_MODE_FAST_AGGREGATE, nullptr, nullptr, status};   // HOST pointers: a shard is its slice
    std::vector<int> rcs(G, MBLS_OK); std::vector<std::thread> th;
    std::vector<const void*> d_send(G, nullptr); std::vector<void*> d_recv(G, nullptr); std::vector<hipStream_t> st(G, nullptr);
    auto work = [&](uint64_t g) {
        mbls_ctx* c = m->ctx[g];
        const uint64_t lo = 64 * W * g < n ? 64 * W * g : n, hi = 64 * W * (g + 1) < n ? 64 * W * (g + 1) : n, cnt = hi - lo;
        mbls_lock lk2(c->mu);
        if (hipSetDevice(c->device) != hipSuccess) { rcs[g] = MBLS_ERR_DEVICE; return; }
        if (m->bm_words_cap < W || !m->d_bm_send[g]) {      // (bm_words_cap is raised after the workers have joined)
            if (m->d_bm_send[g]) { (void)hipFree(m->d_bm_send[g]); m->d_bm_send[g] = nullptr; }
            if (m->d_bm_all[g]) { (void)hipFree(m->d_bm_all[g]); m->d_bm_all[g] = nullptr; }
            if (hipMalloc(&m->d_bm_send[g], 8 * W) != hipSuccess || hipMalloc(&m->d_bm_all[g], 8 * W * G) != hipSuccess) { rcs[g] = MBLS_ERR_DEVICE; return; }
        }
        d_send[g] = m->d_bm_send[g]; d_recv[g] = m->d_bm_all[g]; st[g] = c->hs_a;
        if (hipMemsetAsync(m->d_bm_send[g], 0, 8 * W, c->hs_a) != hipSuccess) { rcs[g] = MBLS_ERR_DEVICE; return; }
        if (!cnt) return;
        const batch sh = slice(all, lo, hi);
        std::vector<uint8_t> res;
        try { res.resize(cnt); } catch (...) { rcs[g] = MBLS_ERR_DEVICE; return; }
        rcs[g] = verify_host(c, sh.d_sigs, sh.ms, nullptr, sh.ks.d_pks, fmt, nullptr, nullptr, sh.ks.d_off, cnt, k, MBLS_MODE_FAST_AGGREGATE, res.data(), sh.d_status);
        if (rcs[g]) return;
        // the shard's result bytes are still in the context's staging buffer (slot 4 of verify_host): pack them where they are
        hipLaunchKernelGGL(k_pack, dim3(nblk(cnt)), dim3(WG), 0, c->hs_a, (const uint8_t*)c->stage[4].p, m->d_bm_send[g], cnt);
        if (hipGetLastError() != hipSuccess) rcs[g] = MBLS_ERR_DEVICE;
    };
    try { for (uint64_t g = 1; g < G; g++) th.emplace_back(work, g); } catch (...) { for (auto& t : th) t.join(); snprintf(m->err, sizeof(m->err), "cannot start a host thread"); return MBLS_ERR_DEVICE; }
    work(0);
    for (auto& t : th) t.join();
    for (uint64_t g = 0; g < G; g++)
        if (rcs[g]) { snprintf(m->err, sizeof(m->err), "device %d (shard %llu): %s", m->ctx[g]->device, (unsigned long long)g, m->ctx[g]->err); m->bm_words_cap = 0; return rcs[g]; }
    if (m->bm_words_cap < W) m->bm_words_cap = W;
    int rc = multi_allgather(m, d_send, d_recv, 8 * W, st); if (rc) return rc;
    if (bitmap) {
        if (hipSetDevice(m->ctx[0]->device) != hipSuccess || hipMemcpy(bitmap, m->d_bm_all[0], 8 * words, hipMemcpyDeviceToHost) != hipSuccess) {
            snprintf(m->err, sizeof(m->err), "bitmap download failed"); return MBLS_ERR_DEVICE;
        }
    }
    return MBLS_OK;
}
extern "C" const uint64_t* mbls_multi_device_bitmap(mbls_multi* m, int g) { return (m && g >= 0 && g < (int)m->ctx.size()) ? m->d_bm_all[g] : nullptr; }
extern "C" int mbls_multi_keytable_create(mbls_multi* m, uint64_t capacity_hint, mbls_multi_keytable** out) {
    if (!m || !out) return MBLS_ERR_ARGUMENT;
    mbls_multi_keytable* t = new (std::nothrow) mbls_multi_keytable();
    if (!t) return MBLS_ERR_DEVICE;
    t->m = m;
    for (mbls_ctx* c : m->ctx) {
        mbls_keytable* x = nullptr;
        int rc = mbls_keytable_create(c, capacity_hint, &x);
        if (rc) { for (mbls_keytable* y : t->tab) mbls_keytable_destroy(y); delete t; return rc; }
        t->tab.push_back(x);
    }
    *out = t; return MBLS_OK;
}
extern "C" void mbls_multi_keytable_destroy(mbls_multi_keytable* t) {
    if (!t) return;
    for (mbls_keytable* x : t->tab) mbls_keytable_destroy(x);
    delete t;
}
extern "C" mbls_keytable* mbls_multi_keytable_replica(mbls_multi_keytable* t, int i) { return (t && i >= 0 && i < (int)t->tab.size()) ? t->tab[i] : nullptr; }
extern "C" uint64_t mbls_multi_keytable_size(const mbls_multi_keytable* t) { return (t && !t->tab.empty()) ? mbls_keytable_size(t->tab[0]) : 0; }
// the same keys, decoded on every device side by side (the indices are the same everywhere); errs as mbls_keytable_append
extern "C" int mbls_multi_keytable_append(mbls_multi_keytable* t, const uint8_t* pks, int fmt, int validate, uint64_t n, uint64_t* first_index, uint8_t* errs) {
    if (!t || !t->m) return MBLS_ERR_ARGUMENT;
    mbls_multi* m = t->m;
    std::lock_guard<std::mutex> lk(m->mu);
    const size_t G = t->tab.size();
    std::vector<int> rcs(G, MBLS_OK); std::vector<uint64_t> first(G, 0);
    std::vector<std::vector<uint8_t>> e(G);
    std::vector<std::thread> th;
    // all or nothing: every replica's size as it is now -- whatever fails below (a worker that could not be started, an append that failed after its records
    // were already published: the stream synchronisation or the download of errs), ALL replicas go back to it, so that indices stay equal everywhere
    std::vector<uint64_t> size0(G);
    for (size_t g = 0; g < G; g++) size0[g] = t->tab[g]->size;
    auto rollback = [&]() { for (size_t g = 0; g < G; g++) if (t->tab[g]->size > size0[g]) keytable_truncate(t->tab[g], size0[g]); };
    auto work = [&](size_t g) {
        uint8_t* eg = errs;
        if (g) { try { e[g].resize(n ? n : 1); } catch (...) { rcs[g] = MBLS_ERR_DEVICE; return; } eg = e[g].data(); }
        rcs[g] = mbls_keytable_append(t->tab[g], pks, fmt, validate, n, &first[g], eg);
    };
    try { for (size_t g = 1; g < G; g++) th.emplace_back(work, g); }
    catch (...) { for (auto& x : th) x.join(); rollback(); snprintf(m->err, sizeof(m->err), "could not start a worker thread"); return MBLS_ERR_DEVICE; }
    work(0);
    for (auto& x : th) x.join();
    int bad = MBLS_OK;
    for (size_t g = 0; g < G && !bad; g++) {
        if (rcs[g]) { snprintf(m->err, sizeof(m->err), "device %d: %s", m->ctx[g]->device, m->ctx[g]->err); bad = rcs[g]; }
        else if (first[g] != first[0] || (g && n && memcmp(e[g].data(), errs, n) != 0)) { snprintf(m->err, sizeof(m->err), "replicas of the key table disagree (device %d)", m->ctx[g]->device); bad = MBLS_ERR_DEVICE; }
    }
    if (bad) { rollback(); return bad; }      // (the size is host-side state: the dropped records are simply overwritten by the next append)
    if (first_index) *first_index = first[0];
    return MBLS_OK;
}
extern "C" int mbls_multi_fast_aggregate_verify_batch_indexed(mbls_multi* m, const mbls_multi_keytable* t, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len,
        const uint64_t* moff, const uint32_t* idx, const uint32_t* off, uint64_t n, uint32_t k, uint8_t* results, uint32_t* status) {
    if (!t) return MBLS_ERR_ARGUMENT;
    return multi_run(m, t, sigs, msgs, msg_len, moff, nullptr, MBLS_PK_UNCOMPRESSED, idx, off, n, k, MBLS_MODE_FAST_AGGREGATE, results, status);
}

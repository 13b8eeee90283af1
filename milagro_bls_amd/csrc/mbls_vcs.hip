// mbls_vcs.hip -- the key phase of verify_multiple over committee spans (include/mbls.h, mbls_verify_multiple_committee_span_msgtable*; rules: mbls_vcs.h) and the
// functions that enqueue it (mbls_vcs_launch.h). A translation unit of its own, for the reason mbls_cms.hip is one: its code object carries its own copies of the
// generated routines the key sum calls, and the code objects of mbls_kernels.hip and mbls_cms.hip stay what they are without these entries.
//   k_vcs_expand       one wave per set: a single-key set's one index, otherwise wave_cms_expand unchanged -> direct list, missing list, record
//   k_aggregate_vcs_d  split factor 1, the throughput form: lane_aggregate_cms, one lane per set, the status word cut by vmc_key_status
//   k_vcs_partial_d    split factor P > 1: one lane per (set, list, chunk) sums its chunk with the generated indexed key sum into a workspace item of its own
//   k_vcs_combine      one lane per set: missing partials, negate, cached sums of the masked segments, direct partials -> the set's APK slots and status bits
#include <hip/hip_runtime.h>
#include "mbls_vcs_launch.h"
#include "mbls_cms_lanes.h"

#if defined(MBLS_NO_ASM) || defined(MBLS_NO_FP2_ASM) || defined(MBLS_NO_LDS_STATE)
#error "libmbls_hip.so cannot be built with MBLS_NO_ASM / MBLS_NO_FP2_ASM / MBLS_NO_LDS_STATE: the host side depends on the generated routines"
#endif
#if defined(__HIP_DEVICE_COMPILE__) && !MBLS_DEVICE_ASM
#error "device pass without the generated routines"
#endif

#define VCS_WG 64
// one wave per SIMD, like the key-sum kernels of mbls_kernels.hip: the generated routine owns 512 registers per lane
#define VCS_LB __launch_bounds__(VCS_WG, 1)

// Set i on the 64 lanes of one wave. The offsets are read and checked first; a range of exactly one id is the only one whose id is looked at here, and only for
// bit 31. Everything else -- a malformed range included -- is wave_cms_expand's, which reads in the span section's order and rejects a bit-31 id among several as
// an id at or above the count.
__global__ void __launch_bounds__(VCS_WG) k_vcs_expand(const uint32_t* crecs, uint64_t ccount, const uint32_t* members, const uint32_t* cmt_ids, uint64_t n_cmt_ids,
                                                       const uint32_t* cmt_off, const uint8_t* bits, uint32_t bits_stride, int mode, uint32_t* list, uint64_t stride,
                                                       uint32_t* item_recs, uint64_t n) {
    const uint64_t i = blockIdx.x; if (i >= n) return;
    const uint32_t off_lo = cmt_off[i], off_hi = cmt_off[i + 1];
    uint32_t q = 0;
    if (cms_range_ok(off_lo, off_hi, n_cmt_ids, &q) && q == 1u) {
        const uint32_t id = cmt_ids[off_lo];
        if (vcs_is_single(q, id)) {
            if (threadIdx.x == 0) vcs_single_item(id, list + stride * i, item_recs + (uint64_t)MBLS_CMS_REC_DWORDS * i);
            return;
        }
    }
    wave_cms_expand(i, threadIdx.x, crecs, ccount, members, cmt_ids, n_cmt_ids, cmt_off, bits, bits_stride, mode, list, stride, item_recs);
}
__global__ void VCS_LB k_aggregate_vcs_d(mbls_ws ws, const uint32_t* recs, uint64_t tsize, const uint32_t* list, uint64_t stride, const uint32_t* item_recs,
                                         const uint32_t* crecs, const uint32_t* cmt_ids, const uint32_t* cmt_off, uint32_t* park, uint64_t park_stride,
                                         uint32_t* status, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * VCS_WG + threadIdx.x; if (i >= n) return;
#if MBLS_DEVICE_ASM            // (the host pass does not see the body)
    uint32_t st = vmc_key_status(lane_aggregate_cms(ws, i, threadIdx.x, recs, tsize, list, stride, item_recs, crecs, cmt_ids, cmt_off, park, park_stride));
    if (st) atomicOr(status + i, st);
#endif
}
// Lane g = (2 i + list) P + p sums chunk p of set i's missing (list 0) or direct (list 1) list into the APK slots of workspace item base + g: lane_aggregate_d<true>
// unchanged, verify mode (neither the empty chunk nor a sum at infinity is flagged; an empty chunk leaves infinity). The lanes of a wave hold consecutive items,
// as the routine's addressing wants. Every lane writes its status word, so st_sub needs no clearing.
__global__ void VCS_LB k_vcs_partial_d(mbls_ws ws, uint64_t base, uint32_t P, const uint32_t* recs, uint64_t tsize, const uint32_t* list, uint64_t stride,
                                       const uint32_t* item_recs, uint32_t* st_sub, uint64_t lanes) {
    const uint64_t g = (uint64_t)blockIdx.x * VCS_WG + threadIdx.x; if (g >= lanes) return;
#if MBLS_DEVICE_ASM
    const uint64_t i = vcs_lane_set(g, P);
    const uint32_t which = vcs_lane_list(g, P), p = vcs_lane_chunk(g, P);
    const uint32_t* rec = item_recs + (uint64_t)MBLS_CMS_REC_DWORDS * i;
    const uint32_t n_direct = rec[0], n_missing = rec[1];
    const uint32_t L = which ? n_direct : n_missing;
    const uint32_t lo = vcs_chunk_lo(L, P, p), hi = vcs_chunk_lo(L, P, p + 1u);
    const uint32_t* first = list + stride * i + (which || !n_missing ? 0u : cms_missing_first(stride, n_missing)) + lo;
    st_sub[g] = lane_aggregate_d<true>(ws, base + g, first, hi - lo, MBLS_MODE_VERIFY, threadIdx.x, recs, tsize);
#endif
}
MBLS_FN void vcs_add_item(g1j* acc, const mbls_ws& ws, uint64_t t) {
    g1j p; p.x = ws_ld(ws, MBLS_SLOT_APK, t); p.y = ws_ld(ws, MBLS_SLOT_APK + 1, t); p.z = ws_ld(ws, MBLS_SLOT_APK + 2, t);
    g1_add(acc, acc, &p);
}
// Set i from its 2 P partial sums, by the compiled group law alone (g1_add: equal operands double, opposite operands give infinity, an infinite operand leaves the
// other): the missing partials, negated, plus the cached sum of every masked segment's committee, plus the direct partials. The status bits are the direct
// partials' alone, cut by vmc_key_status: the missing list names members of eligible committees, whose sum can report none (mbls_cms.h). The partial sum of an
// EMPTY chunk is infinity and is not added: at full participation both lists are empty and the lane does what the one-lane form does, the cached sums alone (an
// addition by the compiled group law costs about as much as two keys of the generated key sum: 32 of them for nothing were 0.5 ms of a 5 ms block).
__global__ void __launch_bounds__(VCS_WG) k_vcs_combine(mbls_ws ws, uint64_t base, uint32_t P, const uint32_t* item_recs, const uint32_t* crecs, const uint32_t* cmt_ids,
                                                        const uint32_t* cmt_off, const uint32_t* st_sub, uint32_t* status, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * VCS_WG + threadIdx.x; if (i >= n) return;
    const uint32_t* rec = item_recs + (uint64_t)MBLS_CMS_REC_DWORDS * i;
    const uint64_t mask = (uint64_t)rec[2] | ((uint64_t)rec[3] << 32);
    const uint32_t n_direct = rec[0], n_missing = rec[1];
    const uint64_t g0 = vcs_lane_of(i, 0u, 0u, P), g1 = vcs_lane_of(i, 1u, 0u, P);
    g1j acc; g1_set_inf(&acc);
    if (mask) {
        for (uint32_t p = 0; p < P; p++)
            if (vcs_chunk_lo(n_missing, P, p) != vcs_chunk_lo(n_missing, P, p + 1u)) vcs_add_item(&acc, ws, base + g0 + p);
        g1_neg(&acc, &acc);
        const uint32_t* ids = cmt_ids + cmt_off[i];
        for (uint32_t t = 0; t < MBLS_CMS_MAX_COMMITTEES; t++) {
            if (!((mask >> t) & 1ull)) continue;
            const uint32_t* sum = crecs + (uint64_t)MBLS_CMT_REC_DWORDS * ids[t] + MBLS_CMT_REC_SUM;
            g1j full;
#pragma unroll
            for (int u = 0; u < 12; u++) { full.x[u] = sum[u]; full.y[u] = sum[12 + u]; full.z[u] = sum[24 + u]; }
            g1_add(&acc, &acc, &full);
        }
    }
    uint32_t st = 0;
    for (uint32_t p = 0; p < P; p++) {
        if (vcs_chunk_lo(n_direct, P, p) != vcs_chunk_lo(n_direct, P, p + 1u)) vcs_add_item(&acc, ws, base + g1 + p);
        st |= st_sub[g1 + p];
    }
    ws_st(ws, MBLS_SLOT_APK, i, acc.x); ws_st(ws, MBLS_SLOT_APK + 1, i, acc.y); ws_st(ws, MBLS_SLOT_APK + 2, i, acc.z);
    st = vmc_key_status(st);
    if (st) atomicOr(status + i, st);
}

void mbls_vcs_launch_expand(const uint32_t* crecs, uint64_t ccount, const uint32_t* members, const uint32_t* cmt_ids, uint64_t n_cmt_ids, const uint32_t* cmt_off,
                            const uint8_t* bits, uint32_t bits_stride, int mode, uint32_t* list, uint64_t stride, uint32_t* item_recs, uint64_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_vcs_expand, dim3((unsigned)n), dim3(VCS_WG), 0, s, crecs, ccount, members, cmt_ids, n_cmt_ids, cmt_off, bits, bits_stride, mode, list, stride,
                       item_recs, n);
}
void mbls_vcs_launch_aggregate(mbls_ws ws, const uint32_t* recs, uint64_t tsize, const uint32_t* list, uint64_t stride, const uint32_t* item_recs, const uint32_t* crecs,
                               const uint32_t* cmt_ids, const uint32_t* cmt_off, uint32_t* park, uint64_t park_stride, uint32_t* status, uint64_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_aggregate_vcs_d, dim3((unsigned)((n + VCS_WG - 1) / VCS_WG)), dim3(VCS_WG), 0, s, ws, recs, tsize, list, stride, item_recs, crecs, cmt_ids, cmt_off,
                       park, park_stride, status, n);
}
void mbls_vcs_launch_split(mbls_ws ws, uint64_t base, uint32_t P, const uint32_t* recs, uint64_t tsize, const uint32_t* list, uint64_t stride, const uint32_t* item_recs,
                           const uint32_t* crecs, const uint32_t* cmt_ids, const uint32_t* cmt_off, uint32_t* st_sub, uint32_t* status, uint64_t n, hipStream_t s) {
    const uint64_t lanes = vcs_extra_items(n, P);
    hipLaunchKernelGGL(k_vcs_partial_d, dim3((unsigned)((lanes + VCS_WG - 1) / VCS_WG)), dim3(VCS_WG), 0, s, ws, base, P, recs, tsize, list, stride, item_recs, st_sub, lanes);
    hipLaunchKernelGGL(k_vcs_combine, dim3((unsigned)((n + VCS_WG - 1) / VCS_WG)), dim3(VCS_WG), 0, s, ws, base, P, item_recs, crecs, cmt_ids, cmt_off,
                       (const uint32_t*)st_sub, status, n);
}

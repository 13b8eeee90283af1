// mbls_vbg.hip -- the grouped route of mbls_verify_multiple_batches_committee_msgtable* (include/mbls.h; rules: mbls_vbg.h): one Miller loop per distinct
// (batch, table entry) pair. A translation unit of its own, for the reason mbls_cms.hip and mbls_vcs.hip are: its code object carries its own copy of the generated
// G1 tree routine, and the code object of mbls_kernels.hip stays what it is without these entries.
//   k_vbg_group     one wave per batch: leaders, group numbers, ranks -> positions, ranges, batch-local group records, group counts (no atomics tickets)
//   k_vbg_scatter   one lane per set: the blinded key -> its position
//   k_vbg_key_tree  one level of the per-group key sums over the positions (the twin of k_g1_seg_tree_d on ranges stated per position: positions have holes)
//   k_vbg_heads     the Miller items: [0, B) the (S_b, -G1) pairs, [B, B + bound) the groups -- H from the table, the key from the head of the group's range
//   k_vbg_gather    one lane per batch: pair value and group product -> the tail's items; table faults and overflow -> the batch's word
//   k_vbg_mark      _locate: mbls_vsl.h's rule with the set's BATCH in the place of the call
#include <hip/hip_runtime.h>
#include "mbls_vbg_launch.h"
#include "mbls_vsl.h"
#include "mbls_vmt.h"

#if defined(MBLS_NO_ASM) || defined(MBLS_NO_FP2_ASM) || defined(MBLS_NO_LDS_STATE)
#error "libmbls_hip.so cannot be built with MBLS_NO_ASM / MBLS_NO_FP2_ASM / MBLS_NO_LDS_STATE: the host side depends on the generated routines"
#endif
#if defined(__HIP_DEVICE_COMPILE__) && !MBLS_DEVICE_ASM
#error "device pass without the generated routines"
#endif

#define MBLS_SLOT_S 25             // 6 Fp: the Jacobian G2 sums of the blinded signatures (mbls_kernels.hip; the generated G2 tree routine's slots 25..30, mbls_lanes.h)
#define VBG_WG 64
#define VBG_HB 256
// one wave per SIMD where a generated routine runs, like the tree kernels of mbls_kernels.hip
#define VBG_LB __launch_bounds__(VBG_WG, 1)

static __device__ __forceinline__ uint64_t vbg_gid() { return (uint64_t)blockIdx.x * VBG_WG + threadIdx.x; }
static __device__ __forceinline__ uint32_t vbg_below(uint64_t mask, uint32_t lane) { return (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)); }

// Batch b on the 64 lanes of one wave (mbls_vbg.h, THE GROUPING). First the sets the batch owns are counted -- and those of them that name nothing flagged --;
// a batch that is not sound (vbg_batch_sound) stops there with no group. Every index of the arrays over the sets lies in the batch's own sound range [lo, hi),
// hi <= n: positions are lo + (a count of the batch's valid sets), group records lo + (a count of its leaders).
__global__ void __launch_bounds__(VBG_WG) k_vbg_group(const uint32_t* msg_idx, uint64_t T, const uint32_t* off, uint32_t spb, uint64_t B, uint64_t n, const uint32_t* map,
                                                      uint32_t* pos, uint32_t* rlo, uint32_t* rhi, uint32_t* head, uint32_t* entry, uint32_t* gcount, uint32_t* status) {
    __shared__ uint32_t s_idx[MBLS_VBG_MAX_SETS], s_leader[MBLS_VBG_MAX_SETS], s_rank[MBLS_VBG_MAX_SETS];
    __shared__ uint32_t s_gnum[MBLS_VBG_MAX_SETS], s_size[MBLS_VBG_MAX_SETS], s_start[MBLS_VBG_MAX_SETS];
    const uint64_t b = blockIdx.x; if (b >= B) return;
    const uint32_t lane = threadIdx.x;
    uint64_t lo, hi;
    if (!vmb_range(off, spb, n, b, &lo, &hi)) { if (lane == 0) gcount[b] = 0; return; }
    const uint64_t m = hi - lo;
    uint64_t mine = 0;
    for (uint64_t base = 0; base < m; base += VBG_WG) {
        const uint64_t j = lo + base + lane;
        const bool own = j < hi && (!off || map[j] == (uint32_t)b);
        if (own && !vbg_valid(msg_idx[j], T)) atomicOr(status + j, MBLS_VBG_BAD_MSG);
        mine += (uint64_t)__popcll(__ballot(own));
    }
    if (mine != m) { if (lane == 0) gcount[b] = 0; return; }
    uint32_t G = 0;
    if (!vbg_batch_grouped(m)) {      // every valid set a group of its own, in set order
        for (uint64_t base = 0; base < m; base += VBG_WG) {
            const uint64_t j = lo + base + lane;
            const uint32_t x = j < hi ? msg_idx[j] : MBLS_VBG_NONE;
            const bool v = j < hi && vbg_valid(x, T);
            const uint64_t mask = __ballot(v);
            if (v) {
                const uint32_t g = G + vbg_below(mask, lane), p = (uint32_t)(lo + g);
                pos[j] = p; rlo[p] = p; rhi[p] = p + 1u; head[lo + g] = p; entry[lo + g] = x;
            }
            G += (uint32_t)__popcll(mask);
        }
        if (lane == 0) gcount[b] = G;
        return;
    }
    const uint32_t mm = (uint32_t)m;
    for (uint32_t j = lane; j < mm; j += VBG_WG) s_idx[j] = msg_idx[lo + j];
    __syncthreads();
    // leaders, ranks and sizes; the leaders of a step take the next group numbers in lane order
    for (uint32_t base = 0; base < mm; base += VBG_WG) {
        const uint32_t j = base + lane;
        uint32_t l = MBLS_VBG_NONE, r = 0, sz = 0;
        const bool v = j < mm && vbg_lane_walk(s_idx, mm, j, T, &l, &r, &sz);
        const bool lead = v && l == j;
        const uint64_t mask = __ballot(lead);
        if (j < mm) { s_leader[j] = v ? l : MBLS_VBG_NONE; s_rank[j] = r; }
        if (lead) { const uint32_t g = G + vbg_below(mask, lane); s_gnum[j] = g; s_size[g] = sz; entry[lo + g] = s_idx[j]; }
        G += (uint32_t)__popcll(mask);
    }
    __syncthreads();
    // the starts: the exclusive scan of the sizes in group order, 64 groups per step
    uint32_t run = 0;
    for (uint32_t base = 0; base < G; base += VBG_WG) {
        const uint32_t g = base + lane;
        const uint32_t v = g < G ? s_size[g] : 0u;
        uint32_t incl = v;
        for (uint32_t d = 1; d < VBG_WG; d *= 2) { const uint32_t up = __shfl_up(incl, d, VBG_WG); if (lane >= d) incl += up; }
        if (g < G) { s_start[g] = run + incl - v; head[lo + g] = (uint32_t)(lo + run + incl - v); }
        run += __shfl(incl, VBG_WG - 1, VBG_WG);
    }
    __syncthreads();
    for (uint32_t j = lane; j < mm; j += VBG_WG) {
        const uint32_t l = s_leader[j]; if (l == MBLS_VBG_NONE) continue;
        const uint32_t g = s_gnum[l], first = (uint32_t)(lo + s_start[g]), p = first + s_rank[j];
        pos[lo + j] = p; rlo[p] = first; rhi[p] = first + s_size[g];
    }
    if (lane == 0) gcount[b] = G;
}
// set i's blinded key (slot APK, the Jacobian form k_blind_g1_d leaves) moves to position item pbase + pos[i]; a set that stands nowhere moves nothing
__global__ void __launch_bounds__(VBG_WG) k_vbg_scatter(mbls_ws ws, const uint32_t* pos, uint64_t n, uint64_t pbase) {
    const uint64_t i = vbg_gid(); if (i >= n) return;
    const uint32_t p = pos[i];
    if (p == MBLS_VBG_NONE || (uint64_t)p >= n) return;
    const uint32_t* src = ws.w + (uint64_t)MBLS_SLOT_APK * 12 * ws.stride + i;
    uint32_t* dst = ws.w + (uint64_t)MBLS_SLOT_APK * 12 * ws.stride + pbase + p;
#pragma unroll 12
    for (int w = 0; w < 36; w++) dst[(uint64_t)w * ws.stride] = src[(uint64_t)w * ws.stride];
}
// One level of the per-group sums of the blinded keys (slot APK of the positions; wp = the workspace seen from the first position): position p takes its partner
// p + half inside its group's range [rlo[p], rhi[p]) (vmb_takes_partner); holes and lanes without a partner at this level return before the routine.
__global__ void VBG_LB k_vbg_key_tree(mbls_ws wp, const uint32_t* rlo, const uint32_t* rhi, uint64_t n, uint64_t half) {
#if MBLS_DEVICE_ASM
    const uint64_t p = vbg_gid(); if (p >= n) return;
    const uint64_t lo = rlo[p], hi = rhi[p];
    if (lo == MBLS_VBG_NONE || !(lo <= p && p < hi && hi <= n)) return;
    if (!vmb_takes_partner(p, lo, hi, half)) return;
    g1_tree_d_call(wp, p, half, threadIdx.x);
#endif
}
// Miller item t of B + bound. t < B: batch t's signature pair, k_vmb_sigpair_setup's operands -- H = S_t (slot S at the head of its range; infinity for an empty
// or faulty range), APK = -G1. Otherwise global group r = t - B: live (vbg_group_live) -- H <- the table entry its batch-local record names (a flagged entry
// rejects the batch: some set of it names the entry), APK <- the sum at the head of its range, imap[r] <- its batch; idle -- the private entry, the point at
// infinity, 1 in slot F (what a wave that returns early leaves for the product tree), imap[r] <- none. Every slot the Miller loops read is written here.
__global__ void __launch_bounds__(VBG_HB) k_vbg_heads(mbls_ws ws, const uint32_t* tab, uint64_t tstride, const uint32_t* flags, uint64_t T, const uint32_t* goff,
                                                      const uint32_t* head, const uint32_t* entry, const uint32_t* off, uint32_t spb, uint64_t B, uint64_t n,
                                                      uint64_t bound, uint64_t pbase, uint32_t* imap, uint32_t* st_batch, uint32_t* live) {
    const uint64_t t = (uint64_t)blockIdx.x * VBG_HB + threadIdx.x; if (t >= B + bound) return;
    if (t == 0) { const uint64_t D = goff[B]; live[0] = (uint32_t)(B + (D < bound ? D : bound)); }      // the items the Miller forms walk (mbls_vmt.h vmt_wave_idle)
    uint64_t lo, hi;
    if (t < B) {
        (void)vmb_range(off, spb, n, t, &lo, &hi);
        const bool some = hi > lo;
        const uint64_t it = some ? lo : 0;                            // (item 0 exists in every workspace: an empty range reads it and keeps nothing)
        g2j o; g2_set_inf(&o);
        g2j sg; sg.x = ws_ld2(ws, MBLS_SLOT_S, it); sg.y = ws_ld2(ws, MBLS_SLOT_S + 2, it); sg.z = ws_ld2(ws, MBLS_SLOT_S + 4, it);
        ws_st2(ws, MBLS_SLOT_H, t, fp2_select(some, sg.x, o.x)); ws_st2(ws, MBLS_SLOT_H + 2, t, fp2_select(some, sg.y, o.y)); ws_st2(ws, MBLS_SLOT_H + 4, t, fp2_select(some, sg.z, o.z));
        ws_st(ws, MBLS_SLOT_APK, t, fp_load_const(MBLS_G1_X)); ws_st(ws, MBLS_SLOT_APK + 1, t, fp_load_const(MBLS_G1_NEG_Y)); ws_st(ws, MBLS_SLOT_APK + 2, t, fp_one());
        return;
    }
    const uint64_t r = t - B;
    uint64_t b = 0;
    bool some = vbg_group_live(goff, B, bound, r, &b);
    uint32_t idx = MBLS_VMT_NO_ENTRY; uint64_t p = 0;
    if (some) {
        some = vmb_range(off, spb, n, b, &lo, &hi);
        const uint64_t g = r - goff[b];
        some = some && lo + g < hi;                                   // (a batch has at most as many groups as sets: k_vbg_group wrote this record)
        if (some) { idx = entry[lo + g]; p = head[lo + g]; some = (uint64_t)idx < T && p < n; }
    }
    if (!some) { idx = MBLS_VMT_NO_ENTRY; p = 0; }
    const uint32_t st = lane_h_gather(ws, t, tab, tstride, flags, idx, T);
    const uint64_t it = pbase + p;                                    // (the first position exists in every such workspace: an idle item reads it and keeps nothing)
    g1j o; g1_set_inf(&o);
    g1j a; a.x = ws_ld(ws, MBLS_SLOT_APK, it); a.y = ws_ld(ws, MBLS_SLOT_APK + 1, it); a.z = ws_ld(ws, MBLS_SLOT_APK + 2, it);
    ws_st(ws, MBLS_SLOT_APK, t, fp_select(some, a.x, o.x)); ws_st(ws, MBLS_SLOT_APK + 1, t, fp_select(some, a.y, o.y)); ws_st(ws, MBLS_SLOT_APK + 2, t, fp_select(some, a.z, o.z));
    imap[r] = some ? (uint32_t)b : MBLS_VBG_NONE;
    if (!some) {
        fp12 f; fp12_set_one(&f);
        const fp* one = &f.c0.c0.c0;
        for (int u = 0; u < 12; u++) ws_st(ws, MBLS_SLOT_F + u, t, one[u]);
    }
    if (some && st) atomicOr(st_batch + b, st);
}
// item `to` <- the Miller value of item `from` (12 Fp, word for word); from = none: 1
static __device__ __forceinline__ void vbg_copy_f(const mbls_ws& ws, bool some, uint64_t from, uint64_t to) {
    fp12 f; fp12_set_one(&f);
    const fp* one = &f.c0.c0.c0;
    for (int u = 0; u < 12; u++) ws_st(ws, MBLS_SLOT_F + u, to, some ? ws_ld(ws, MBLS_SLOT_F + u, from) : one[u]);
}
// Batch b behind the products' tree: the value of its signature pair (Miller item b) -> tail item b, the product of its group items (left at its first group
// item B + goff[b]; 1 for a batch without groups) -> tail item B + b. Its word takes k_vmb_gather's verdict on the table -- a faulty range, or a range of which
// another batch owns a set, rejects it (MBLS_ST_BAD_PK_ENCODING) -- and the overflow rule (vbg_overflow: MBLS_ST_BAD_MSG_RANGE, and no group item is read).
__global__ void __launch_bounds__(VBG_WG) k_vbg_gather(mbls_ws ws, const uint32_t* goff, const uint32_t* off, uint32_t spb, uint64_t B, uint64_t n, uint64_t bound,
                                                       uint64_t tail, uint32_t* st_batch, const uint32_t* owned) {
    const uint64_t b = vbg_gid(); if (b >= B) return;
    uint64_t lo, hi;
    uint32_t st = 0;
    if (!vmb_range(off, spb, n, b, &lo, &hi)) st |= MBLS_ST_BAD_PK_ENCODING;
    if (!vmb_owns_all(off ? owned : nullptr, b, lo, hi)) st |= MBLS_ST_BAD_PK_ENCODING;
    const bool over = vbg_overflow(goff, b, bound);
    if (over) st |= MBLS_ST_BAD_MSG_RANGE;
    const bool some = !over && goff[b + 1] > goff[b];
    vbg_copy_f(ws, true, b, tail + b);
    vbg_copy_f(ws, some, B + (some ? (uint64_t)goff[b] : 0), tail + B + b);
    if (st) atomicOr(st_batch + b, st);
}
// _locate, after the per-batch tail, one lane per set (wsa = the workspace seen from the first shadow item A(0)): k_vml_mark's ownership and verdict lookup, on
// the word vsl_own_word gives -- the grouped route reports a flagged entry in the BATCH's word only, so the set's own word gets the bit here. A candidate names
// a sound entry: its point goes from the table to slot H of A(i), which completes the pair (H(m_i), [r_i] apk_i).
__global__ void __launch_bounds__(VBG_WG) k_vbg_mark(mbls_ws wsa, const uint32_t* tab, uint64_t tstride, const uint32_t* flags, const uint32_t* msg_idx, uint64_t T,
                                                     const uint32_t* map, const uint32_t* off, uint32_t spb, uint64_t B, uint64_t n, const uint32_t* st_set,
                                                     const uint32_t* owned, const uint8_t* batch_results, uint32_t* cand, uint8_t* set_results, uint32_t* set_status) {
    const uint64_t i = vbg_gid(); if (i >= n) return;
    uint64_t lo = 0, hi = 0, b = 0;
    bool own = vmb_owner_range(map, off, spb, B, n, i, &lo, &hi);
    if (own) { b = off ? map[i] : i / spb; own = vmb_owns_all(off ? owned : nullptr, b, lo, hi); }
    const uint32_t j = msg_idx[i];
    uint32_t st;
    const uint32_t v = vml_mark(own, own && batch_results[b] != 0, vsl_own_word(st_set[i], j, T, flags), &st);
    cand[i] = v == MBLS_VML_CANDIDATE ? 1u : 0u;
    set_results[i] = v == MBLS_VML_TRUE ? 1 : 0;                      // (a candidate stays 0 until its own check has spoken: fail closed)
    if (set_status) set_status[i] = st;
    if (v == MBLS_VML_CANDIDATE) (void)lane_h_gather(wsa, i, tab, tstride, flags, j, T);
}

static inline unsigned vbg_nblk(uint64_t n, unsigned wg) { return (unsigned)((n + wg - 1) / wg); }
void mbls_vbg_launch_group(const uint32_t* msg_idx, uint64_t T, const uint32_t* off, uint32_t spb, uint64_t B, uint64_t n, const uint32_t* map, mbls_vbg_arrays a,
                           uint32_t* status, hipStream_t s) {
    if (!B) return;
    hipLaunchKernelGGL(k_vbg_group, dim3((unsigned)B), dim3(VBG_WG), 0, s, msg_idx, T, off, spb, B, n, map, a.pos, a.rlo, a.rhi, a.head, a.entry, a.gcount, status);
}
void mbls_vbg_launch_scatter(mbls_ws ws, const uint32_t* pos, uint64_t n, uint64_t pbase, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_vbg_scatter, dim3(vbg_nblk(n, VBG_WG)), dim3(VBG_WG), 0, s, ws, pos, n, pbase);
}
void mbls_vbg_launch_key_trees(mbls_ws wp, const uint32_t* rlo, const uint32_t* rhi, uint64_t n, uint32_t levels, hipStream_t s) {
    uint64_t half = 1;
    for (uint32_t l = 0; n && l < levels; l++, half *= 2) hipLaunchKernelGGL(k_vbg_key_tree, dim3(vbg_nblk(n, VBG_WG)), dim3(VBG_WG), 0, s, wp, rlo, rhi, n, half);
}
void mbls_vbg_launch_heads(mbls_ws ws, const uint32_t* tab, uint64_t tstride, const uint32_t* flags, uint64_t T, mbls_vbg_arrays a, const uint32_t* off, uint32_t spb,
                           uint64_t B, uint64_t n, uint64_t bound, uint64_t pbase, uint32_t* imap, uint32_t* st_batch, uint32_t* live, hipStream_t s) {
    if (!(B + bound)) return;
    hipLaunchKernelGGL(k_vbg_heads, dim3(vbg_nblk(B + bound, VBG_HB)), dim3(VBG_HB), 0, s, ws, tab, tstride, flags, T, (const uint32_t*)a.goff, (const uint32_t*)a.head,
                       (const uint32_t*)a.entry, off, spb, B, n, bound, pbase, imap, st_batch, live);
}
void mbls_vbg_launch_gather(mbls_ws ws, mbls_vbg_arrays a, const uint32_t* off, uint32_t spb, uint64_t B, uint64_t n, uint64_t bound, uint64_t tail,
                            uint32_t* st_batch, const uint32_t* owned, hipStream_t s) {
    if (!B) return;
    hipLaunchKernelGGL(k_vbg_gather, dim3(vbg_nblk(B, VBG_WG)), dim3(VBG_WG), 0, s, ws, (const uint32_t*)a.goff, off, spb, B, n, bound, tail, st_batch, owned);
}
void mbls_vbg_launch_mark(mbls_ws wsa, const uint32_t* tab, uint64_t tstride, const uint32_t* flags, const uint32_t* msg_idx, uint64_t T, const uint32_t* map,
                          const uint32_t* off, uint32_t spb, uint64_t B, uint64_t n, const uint32_t* st_set, const uint32_t* owned, const uint8_t* batch_results,
                          uint32_t* cand, uint8_t* set_results, uint32_t* set_status, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_vbg_mark, dim3(vbg_nblk(n, VBG_WG)), dim3(VBG_WG), 0, s, wsa, tab, tstride, flags, msg_idx, T, map, off, spb, B, n, st_set, owned,
                       batch_results, cand, set_results, set_status);
}

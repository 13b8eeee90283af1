// mbls_vmb.h -- the pure segment arithmetic of mbls_verify_multiple_batches* (include/mbls.h): B batches over n sets laid out back to back,
// batch b owning the sets [off[b], off[b + 1]) or k each. Which set takes which partner at which level of the per-batch trees (the G2 sum of
// the blinded signatures, the Fp12 product of the Miller values), which words a batch owns, and what a faulty device-side table turns into.
// A header of its own so that a host compiler can build it for the CPU tests (tests/vmb_emul/mbls_vmb_harness.cpp); the kernels
// k_vmb_set_map, k_g2_seg_tree_d, k_vmb_sigpair_setup, k_vmb_status_fold and k_vmb_gather of mbls_kernels.hip run exactly these.
#ifndef MBLS_VMB_H
#define MBLS_VMB_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define MBLS_VFN static inline __host__ __device__
#else
#define MBLS_VFN static inline
#endif

#define MBLS_VMB_NO_OWNER 0xFFFFFFFFu         // map[j]: no batch owns set j (what the map holds before k_vmb_set_map has spoken)

// batch b's range as the table states it; false: the range is faulty (runs backwards or ends beyond n) and is then EMPTY -- a faulty range
// never becomes a read. Uniform layout (off == NULL): k sets each; the entries check B * k == n before anything runs.
MBLS_VFN bool vmb_range(const uint32_t* off, uint32_t k, uint64_t n, uint64_t b, uint64_t* lo, uint64_t* hi) {
    if (!off) { *lo = (uint64_t)k * b; *hi = *lo + k; return *hi <= n; }
    *lo = off[b]; *hi = off[b + 1];
    if (*hi < *lo || *hi > n) { *hi = *lo = 0; return false; }
    return true;
}
// The map of a ragged layout: every batch with a sound range CLAIMS the sets of its range, one after the other (k_vmb_set_map, one lane per batch, an atomic
// compare-and-swap per set). The first claimant of a set finds "no owner" and leaves its index; every later one finds something else and leaves "shared" -- so
// whatever order the claims arrive in, a set ends up owned by the one batch that claims it, or by nobody when two or more do (tables that run backwards in
// between make ranges overlap). vmb_claim is that step on the word's value.
#define MBLS_VMB_SHARED 0xFFFFFFFEu           // map[j]: two or more batches claim set j -- it belongs to none (batch indices stay below this)
MBLS_VFN uint32_t vmb_claim(uint32_t found, uint32_t b) { return found == MBLS_VMB_NO_OWNER ? b : MBLS_VMB_SHARED; }
// the range set j works in: its owner's (ragged: through the map, which only batches with a sound range have written). false: no owner.
MBLS_VFN bool vmb_owner_range(const uint32_t* map, const uint32_t* off, uint32_t k, uint64_t B, uint64_t n, uint64_t j, uint64_t* lo, uint64_t* hi) {
    if (j >= n) return false;
    if (!off) { if (!k) return false; *lo = (j / k) * k; *hi = *lo + k; return *hi <= n; }
    const uint32_t b = map[j];
    if (b >= B) return false;
    if (!vmb_range(off, k, n, b, lo, hi)) return false;
    return *lo <= j && j < *hi;
}
// one level of a per-batch tree: set j of the range [lo, hi) takes its partner j + half when it stands a multiple of 2 half from the start of
// the range and the partner lies inside it. After the levels half = 1, 2, 4, ... < hi - lo the head of the range holds the whole range.
MBLS_VFN bool vmb_takes_partner(uint64_t j, uint64_t lo, uint64_t hi, uint64_t half) {
    return (j - lo) % (2 * half) == 0 && j + half < hi;
}
// the levels a call enqueues: half = 1, 2, 4, ... < longest, the longest range any batch may have (uniform: k; a device-side table: all n sets)
MBLS_VFN uint32_t vmb_levels(uint64_t longest) { uint32_t l = 0; for (uint64_t half = 1; half < longest; half *= 2) l++; return l; }
// Does batch b own every set of its range ALONE? A set two batches claim is owned by neither (vmb_claim), and trees touch only sets that have an owner, inside
// that owner's range: so a batch that owns every set of its range shares none, was summed from exactly its own sets, and every batch that shares a set owns
// fewer sets than its range holds. owned[b] = the number of sets j with map[j] = b (k_vmb_status_fold counts them, one lane per set). Uniform layout
// (owned == NULL): ranges cannot overlap.
MBLS_VFN bool vmb_owns_all(const uint32_t* owned, uint64_t b, uint64_t lo, uint64_t hi) {
    return !owned || (uint64_t)owned[b] == hi - lo;
}
// host-side validation of a batch table (the host entries refuse the call): B + 1 entries, first 0, non-decreasing, last n; *longest receives the longest range
MBLS_VFN bool vmb_offsets_ok(const uint32_t* off, uint64_t B, uint64_t n, uint64_t* longest) {
    uint64_t m = 0;
    if (off[0] != 0 || off[B] != n) return false;
    for (uint64_t b = 0; b < B; b++) {
        if (off[b + 1] < off[b]) return false;
        if ((uint64_t)(off[b + 1] - off[b]) > m) m = off[b + 1] - off[b];
    }
    if (longest) *longest = m;
    return true;
}
// workspace items a call needs: the sets [0, n), the B (S_b, -G1) pairs [n, n + B), B staging items [n + B, n + 2 B); the lane-pair message
// phase (pair_hash) works on items [0, 2 n)
MBLS_VFN uint64_t vmb_workspace_items(uint64_t n, uint64_t B, bool pair_hash) {
    const uint64_t a = n + 2 * B, h = pair_hash ? 2 * n : n;
    return a > h ? a : h;
}
#endif

// mbls_vmr.h -- the draw order of the verify_multiple*_rng entries, once. The reference's loop (src/aggregates.rs:272-287) tests set i's signature for the
// subgroup BEFORE it draws rand[i] from the caller's generator and returns at the first signature outside G2: a rejected batch leaves the generator after exactly
// as many draws as sets came before the bad one. B batches in one call are B such calls sharing one generator, batch after batch. These functions decide, from
// the status words the signature phase read back, how many scalars `draw` is asked for, which sets they go to, and what locate mode answers for the sets that
// never got one. Pure (no HIP call, no context): a header of its own, like mbls_vmb.h and mbls_vml.h, so that a host compiler can build it for the CPU tests
// (tests/vmr_emul/mbls_vmr_harness.cpp).
#ifndef MBLS_VMR_H
#define MBLS_VMR_H
#include <stdint.h>
#include "../../include/mbls.h"

// the sets of [lo, hi) in front of the first one whose signature the reference's loop stops at (hi - lo: none does); 64-bit positions -- the one-batch entries
// take a size_t n
static inline uint64_t vmr_reach(const uint32_t* st, uint64_t lo, uint64_t hi) {
    for (uint64_t i = lo; i < hi; i++)
        if (st[i] & (MBLS_ST_BAD_SIG_ENCODING | MBLS_ST_SIG_NOT_IN_G2)) return i - lo;
    return hi - lo;
}
// the sets [*lo, *hi) of batch b: a range of the batch table, or spb each
static inline void vmr_batch_range(const uint32_t* boff, uint32_t spb, uint64_t b, uint64_t* lo, uint64_t* hi) {
    *lo = boff ? boff[b] : (uint64_t)spb * b;
    *hi = boff ? boff[b + 1] : *lo + spb;
}
// reach[b] for every batch -> the number of scalars to ask `draw` for
static inline uint64_t vmr_plan(const uint32_t* st, const uint32_t* boff, uint32_t spb, uint64_t B, uint64_t* reach) {
    uint64_t total = 0, lo, hi;
    for (uint64_t b = 0; b < B; b++) { vmr_batch_range(boff, spb, b, &lo, &hi); reach[b] = vmr_reach(st, lo, hi); total += reach[b]; }
    return total;
}
// the drawn scalars, in order, to the sets in front of each batch's reach; the scalar 1 to every other set (its batch is rejected through its status bits
// whatever its pairing product is)
static inline void vmr_spread(const uint64_t* drawn, const uint64_t* reach, const uint32_t* boff, uint32_t spb, uint64_t B, uint64_t* rands) {
    uint64_t at = 0, lo, hi;
    for (uint64_t b = 0; b < B; b++) {
        vmr_batch_range(boff, spb, b, &lo, &hi);
        for (uint64_t i = lo; i < hi; i++) rands[i] = i - lo < reach[b] ? drawn[at++] : 1;
    }
}
// locate mode's closing step: a set at or behind its batch's reach never had a scalar and cannot be examined -- its answer is 0 and its word (set_status is
// optional) what the signature phase found
static inline void vmr_close(const uint32_t* st, const uint64_t* reach, const uint32_t* boff, uint32_t spb, uint64_t B, uint8_t* set_results, uint32_t* set_status) {
    uint64_t lo, hi;
    for (uint64_t b = 0; b < B; b++) {
        vmr_batch_range(boff, spb, b, &lo, &hi);
        for (uint64_t i = lo + reach[b]; i < hi; i++) { set_results[i] = 0; if (set_status) set_status[i] = st[i]; }
    }
}
#endif

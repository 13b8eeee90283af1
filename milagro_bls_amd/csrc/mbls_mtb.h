// mbls_mtb.h -- the index arithmetic of the resident message table (include/mbls.h, "resident message table"): where an entry lives, what a public index maps
// to, how the table grows and how its entries move when it does. A header of its own, like mbls_vms.h and mbls_vsl.h, so that a host compiler can build it for
// the CPU tests (tests/msgtab_emul/mbls_msgtab_harness.cpp); lane_h_gather (mbls_lanes.h: k_h_gather, k_mtb_get) maps an index with exactly mtb_entry,
// k_mtb_relayout of mbls_kernels.hip runs exactly mtb_relayout_entry, and the table's host code sizes and grows its buffers with exactly mtb_stride / mtb_grown.
//
// The layout is the one lane_h_export writes and lane_h_gather reads (mbls_lanes.h): entry-major, dword w of entry e at tab[w * stride + e], one flag word per
// entry. Entry 0 is private: H of the empty message, what an index that names nothing gets. Public index j is entry j + 1. stride = capacity + 1 entries, so a
// table that grows changes its stride: every dword of every entry moves (mtb_relayout_entry), the indices and the entries' contents stay.
#ifndef MBLS_MTB_H
#define MBLS_MTB_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define MBLS_MFN static inline __host__ __device__
#else
#define MBLS_MFN static inline
#endif

#define MBLS_MTB_DWORDS 72                    // MBLS_H_DWORDS: workspace slot H, three Fp2
#define MBLS_MTB_DEFAULT_CAPACITY 1024        // capacity_hint = 0

// entries the buffers hold for a table of `capacity` public entries: the private entry in front
MBLS_MFN uint64_t mtb_stride(uint64_t capacity) { return capacity + 1; }
// the entry a public index names in a table of `size` public entries; an index at or above size (an empty table: every index) names nothing and maps to the
// private entry 0 -- lane_h_gather gives such an item the empty message's point and the bad-range bit
MBLS_MFN uint64_t mtb_entry(uint32_t idx, uint64_t size) { return (uint64_t)idx >= size ? 0 : (uint64_t)idx + 1; }
MBLS_MFN int mtb_names_nothing(uint32_t idx, uint64_t size) { return (uint64_t)idx >= size; }
// where dword w of entry e lives
MBLS_MFN uint64_t mtb_at(uint64_t w, uint64_t stride, uint64_t e) { return w * stride + e; }
// the entry an append's message i goes to when the table holds `size` public entries (its public index is size + i)
MBLS_MFN uint64_t mtb_append_entry(uint64_t size, uint64_t i) { return size + i + 1; }
// the capacity after an append that needs `need` public entries: unchanged while they fit, otherwise doubled (or `need` where that is more)
MBLS_MFN uint64_t mtb_grown(uint64_t capacity, uint64_t need) {
    if (need <= capacity) return capacity;
    return 2 * capacity > need ? 2 * capacity : need;
}
// growth: entry e (0 .. size, the private entry included) of the old buffers to the same entry of the new ones
MBLS_MFN void mtb_relayout_entry(const uint32_t* old_tab, uint64_t old_stride, const uint32_t* old_flags, uint32_t* new_tab, uint64_t new_stride, uint32_t* new_flags,
                                 uint64_t e) {
    for (int w = 0; w < MBLS_MTB_DWORDS; w++) new_tab[mtb_at((uint64_t)w, new_stride, e)] = old_tab[mtb_at((uint64_t)w, old_stride, e)];
    new_flags[e] = old_flags[e];
}
#endif

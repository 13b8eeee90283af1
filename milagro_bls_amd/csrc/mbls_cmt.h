// mbls_cmt.h -- the arithmetic of the committee table (include/mbls.h, "committee table"): which bits of an item's bitfield count, which of the two routes the
// item takes, and where each listed member lands in the item's index list. A header of its own, like mbls_vms.h, mbls_vmt.h and mbls_mtb.h, so that a host
// compiler can build it for the CPU tests (tests/cmt_emul/mbls_cmt_harness.cpp): k_cmt_expand of mbls_kernels.hip runs exactly cmt_selected, cmt_route,
// cmt_listed and cmt_pos -- one lane per member, 64 members per step --, and mbls_plan_committee_route reports from cmt_route.
//
// A committee is an ordered member list of m key-table indices, 1 <= m <= MBLS_CMT_MAX_MEMBERS. An item names a committee and carries a bitfield in SSZ bit order:
// member j signed when (byte[j >> 3] >> (j & 7)) & 1 -- on a little-endian machine bit j & 31 of 32-bit word j >> 5, which is how the kernel reads it (the field
// is 4-byte aligned, its stride a multiple of 4). Bits at positions >= m do not count. With s members selected the item's key sum is either
//   direct:      the sum of the s selected members (s additions), or
//   complement:  the committee's cached full sum minus the sum of the m - s missing members ((m - s) additions and one fix-up addition),
// and the complement is taken when the committee is ELIGIBLE (every member a valid, finite table entry: only then are the BAD_PK_ENCODING / PK_INFINITY bits of
// every subset known to be zero, so the status word does not depend on the route) and it is the cheaper of the two by that count of additions.
#ifndef MBLS_CMT_H
#define MBLS_CMT_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define MBLS_CFN static inline __host__ __device__
#else
#define MBLS_CFN static inline
#endif

#define MBLS_CMT_MAX_MEMBERS 2048u            // include/mbls.h MBLS_COMMITTEE_MAX_MEMBERS
#define MBLS_CMT_STEP 64u                     // members per step of the expansion: one per lane
// a committee's record: [0] first member (position in the table's member array), [1] members, [2] eligible, [3] unused, [4..40) the full sum, Jacobian X, Y, Z in
// the workspace's Montgomery limbs (what the compiled group law adds to)
#define MBLS_CMT_REC_DWORDS 40u
#define MBLS_CMT_REC_SUM 4u
enum { MBLS_CMT_ROUTE_AUTO = 0, MBLS_CMT_ROUTE_DIRECT = 1, MBLS_CMT_ROUTE_COMPLEMENT = 2 };      // mbls_ctx_set_committee_route
#define MBLS_CMT_NO_COMMITTEE 0xFFFFFFFFu     // the one index a device item whose committee id names nothing lists: outside every key table

// 1: the item takes the complement route. m members, s selected, mode as mbls_ctx_set_committee_route
MBLS_CFN int cmt_route(uint32_t m, uint32_t s, int eligible, int mode) {
    if (!eligible || mode == MBLS_CMT_ROUTE_DIRECT || s > m) return 0;
    if (mode == MBLS_CMT_ROUTE_COMPLEMENT) return 1;              // (s = 0 included: full sum minus full sum, infinity, like the empty list's sum)
    return (uint64_t)(m - s) + 1 < (uint64_t)s;
}
// the bits of word w (members 32 w .. 32 w + 31) that name members of a committee of m
MBLS_CFN uint32_t cmt_word_mask(uint32_t m, uint32_t w) {
    const uint32_t lo = 32u * w;
    if (m <= lo) return 0u;
    return m - lo >= 32u ? 0xFFFFFFFFu : (1u << (m - lo)) - 1u;
}
// member j's bit (the caller has checked j < m)
MBLS_CFN int cmt_selected(const uint32_t* words, uint32_t j) { return (int)((words[j >> 5] >> (j & 31u)) & 1u); }
// does member j go into the item's list: the selected members on the direct route, the missing ones on the complement route
MBLS_CFN int cmt_listed(const uint32_t* words, uint32_t j, uint32_t m, int complement) { return j < m && (cmt_selected(words, j) != 0) != (complement != 0); }
// the list position of lane `lane` of a step whose listed lanes are the bits of `ballot`, `out` entries having been written by earlier steps
MBLS_CFN uint32_t cmt_pos(uint32_t out, uint64_t ballot, uint32_t lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    return out + __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
#else
    return out + (uint32_t)__builtin_popcountll(ballot & ((1ull << lane) - 1ull));
#endif
}
MBLS_CFN uint32_t cmt_popcount(uint64_t ballot) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(ballot);
#else
    return (uint32_t)__builtin_popcountll(ballot);
#endif
}
// the selected members of a committee of m, 64 at a time (the count every lane of the wave arrives at)
MBLS_CFN uint32_t cmt_count_selected(const uint32_t* words, uint32_t m) {
    uint32_t s = 0;
    for (uint32_t w = 0; 32u * w < m; w++) s += cmt_popcount((uint64_t)(words[w] & cmt_word_mask(m, w)));
    return s;
}
// The whole expansion of one item as the wave runs it, lane by lane (the host statement of k_cmt_expand; `members` may be null: the list then holds positions
// j instead of key indices). list: room for m entries. Returns the count; *complement receives the route.
MBLS_CFN uint32_t cmt_expand_item(const uint32_t* words, const uint32_t* members, uint32_t m, int eligible, int mode, uint32_t* list, int* complement) {
    const uint32_t s = cmt_count_selected(words, m);
    const int comp = cmt_route(m, s, eligible, mode);
    uint32_t out = 0;
    for (uint32_t base = 0; base < m; base += MBLS_CMT_STEP) {
        uint64_t ballot = 0;
        for (uint32_t lane = 0; lane < MBLS_CMT_STEP; lane++) if (cmt_listed(words, base + lane, m, comp)) ballot |= 1ull << lane;
        for (uint32_t lane = 0; lane < MBLS_CMT_STEP; lane++)
            if ((ballot >> lane) & 1ull) list[cmt_pos(out, ballot, lane)] = members ? members[base + lane] : base + lane;
        out += cmt_popcount(ballot);
    }
    *complement = comp;
    return out;
}
#endif

// mbls_cms.h -- the arithmetic of committee SPANS (include/mbls.h, "committee spans"): an item names q <= MBLS_CMS_MAX_COMMITTEES committees of a committee table and
// carries ONE bitfield, the concatenation of the committees' participation bits (an Electra attestation: committee_bits + aggregation_bits). A header of its own
// beside mbls_cmt.h, in the same host-and-device style, so that a host compiler can build it for the CPU tests (tests/cms_emul/mbls_cms_harness.cpp):
// wave_cms_expand of mbls_cms_lanes.h runs exactly cms_item_ok, cms_count_selected, cms_route, cms_listed, cms_direct_pos and cms_missing_pos -- one lane per
// member, 64 members per step --, and mbls_plan_committee_span reports from cms_plan_item.
//
// Segment t is committee c_t of m_t members; it owns bits [o_t, o_t + m_t) of the field, o_t = m_0 + ... + m_(t-1), M = o_q. Bit order is SSZ, as in mbls_cmt.h:
// bit p is bit p & 31 of 32-bit word p >> 5. Bits at or above M do not count. Every segment takes its own route from cmt_route(m_t, s_t, eligible_t, mode); the
// item's key sum is
//   sum over direct segments of their selected members  +  sum over complement segments of (cached sum of c_t  -  sum of its missing members),
// so the expansion leaves TWO lists per item: the DIRECT list (selected members of direct segments, in (segment, member) order) and the MISSING list (absent
// members of complement segments). Both together never exceed M entries: they share one region of `stride` >= max(M, 1) words, the direct list ascending from
// word 0, the missing list descending from word stride - 1 (entry p at stride - 1 - p; the key sum reads it as the ascending run [stride - n_missing, stride):
// a sum does not depend on the order of its terms).
// ELIGIBLE is the committee record's word [2] as lane_cmt_build (mbls_cmt_lanes.h) sets it at the append: 1 only if the indexed key sum over ALL members reported
// neither BAD_PK_ENCODING nor PK_INFINITY, i.e. every member is a valid, finite table entry. cmt_route sends only eligible committees to the complement, so the
// missing list names such entries alone and its sum can report no status bit: lane_aggregate_cms (mbls_cms_lanes.h) drops that sum's status word on this ground.
// Whoever widens `eligible` has to OR that word into the item's status there.
#ifndef MBLS_CMS_H
#define MBLS_CMS_H
#include "mbls_cmt.h"

#define MBLS_CMS_MAX_COMMITTEES 64u           // include/mbls.h MBLS_SPAN_MAX_COMMITTEES: the mask of complement segments is one 64-bit word
// the per-item record the expansion leaves for the key sum: [0] entries of the direct list, [1] entries of the missing list, [2], [3] the mask of the segments
// that went complement (bit t: segment t; low word first), [4] flags
#define MBLS_CMS_REC_DWORDS 5u
#define MBLS_CMS_FL_NOBODY 1u                 // no member of the whole item is selected
// the point the key sum parks between its two list sums (sum of the masked committees' cached sums minus the missing list's sum): Jacobian X, Y, Z
#define MBLS_CMS_PARK_DWORDS 36u

// the list region of one item, in words: min(8 * bits_stride, 64 * max_members), at least 1 (a malformed item lists one index)
MBLS_CFN uint64_t cms_stride(uint32_t bits_stride, uint32_t max_members) {
    const uint64_t a = (uint64_t)8 * bits_stride, b = (uint64_t)MBLS_CMS_MAX_COMMITTEES * max_members;
    const uint64_t s = a < b ? a : b;
    return s ? s : 1u;
}
// segment t's bit offset in the item's field
MBLS_CFN uint32_t cms_seg_offset(const uint32_t* sizes, uint32_t t) {
    uint32_t o = 0;
    for (uint32_t u = 0; u < t; u++) o += sizes[u];
    return o;
}
// the shape of an item's id range: q in *q, or 0 (malformed) when the offsets run backwards, leave the id array or name more than 64 committees
MBLS_CFN int cms_range_ok(uint32_t off_lo, uint32_t off_hi, uint64_t n_cmt_ids, uint32_t* q) {
    if (off_hi < off_lo || (uint64_t)off_hi > n_cmt_ids || off_hi - off_lo > MBLS_CMS_MAX_COMMITTEES) return 0;
    *q = off_hi - off_lo;
    return 1;
}
// the field covers the item: M bits in bits_bytes bytes
MBLS_CFN int cms_field_ok(uint64_t M, uint64_t bits_bytes) { return M <= 8u * bits_bytes; }
// member j of the segment at bit offset o (the caller has checked j < m): an unaligned position of the field
MBLS_CFN int cms_selected(const uint32_t* words, uint32_t o, uint32_t j) { const uint32_t p = o + j; return (int)((words[p >> 5] >> (p & 31u)) & 1u); }
// the bits of word w that belong to the segment [o, o + m): the masks at both ends
MBLS_CFN uint32_t cms_word_mask(uint32_t o, uint32_t m, uint32_t w) {
    const uint64_t lo = (uint64_t)32u * w, hi = lo + 32u, a = o, b = (uint64_t)o + m;
    if (b <= lo || a >= hi) return 0u;
    uint32_t mask = 0xFFFFFFFFu;
    if (a > lo) mask &= 0xFFFFFFFFu << (uint32_t)(a - lo);
    if (b < hi) mask &= (1u << (uint32_t)(b - lo)) - 1u;
    return mask;
}
// the selected members of the segment [o, o + m), m >= 1 (the count every lane of the wave arrives at)
MBLS_CFN uint32_t cms_count_selected(const uint32_t* words, uint32_t o, uint32_t m) {
    uint32_t s = 0;
    const uint32_t w0 = o >> 5, w1 = (o + m - 1u) >> 5;
    for (uint32_t w = w0; w <= w1; w++) s += cmt_popcount((uint64_t)(words[w] & cms_word_mask(o, m, w)));
    return s;
}
// the route of one segment: the committee entries' own decision
MBLS_CFN int cms_route(uint32_t m, uint32_t s, int eligible, int mode) { return cmt_route(m, s, eligible, mode); }
// does member j of the segment go into a list: the selected members of a direct segment (direct list), the missing ones of a complement segment (missing list)
MBLS_CFN int cms_listed(const uint32_t* words, uint32_t o, uint32_t j, uint32_t m, int complement) {
    return j < m && (cms_selected(words, o, j) != 0) != (complement != 0);
}
// where lane `lane` of a step writes in the item's region: the direct list grows upwards, the missing list downwards from the region's last word
MBLS_CFN uint64_t cms_direct_pos(uint32_t n_direct, uint64_t ballot, uint32_t lane) { return cmt_pos(n_direct, ballot, lane); }
MBLS_CFN uint64_t cms_missing_pos(uint64_t stride, uint32_t n_missing, uint64_t ballot, uint32_t lane) { return stride - 1u - cmt_pos(n_missing, ballot, lane); }
// where the key sum finds the first word of the missing list
MBLS_CFN uint64_t cms_missing_first(uint64_t stride, uint32_t n_missing) { return stride - n_missing; }

// The whole expansion of one WELL-FORMED item as the wave runs it, lane by lane (the host statement of k_cms_expand). sizes / firsts / eligible: the q segments'
// records (firsts[t]: where committee c_t's member list starts in `members`; members may be null: the lists then hold bit positions o_t + j instead of key
// indices). region: `stride` words, stride >= max(M, 1). rec: MBLS_CMS_REC_DWORDS words.
MBLS_CFN void cms_expand_item(const uint32_t* words, const uint32_t* members, const uint32_t* sizes, const uint32_t* firsts, const uint8_t* eligible, uint32_t q, int mode,
                              uint32_t* region, uint64_t stride, uint32_t* rec) {
    uint32_t o = 0, n_direct = 0, n_missing = 0, total = 0;
    uint64_t mask = 0;
    for (uint32_t t = 0; t < q; t++) {
        const uint32_t m = sizes[t];
        const uint32_t s = cms_count_selected(words, o, m);
        const int comp = cms_route(m, s, eligible[t] != 0, mode);
        for (uint32_t base = 0; base < m; base += MBLS_CMT_STEP) {
            uint64_t ballot = 0;
            for (uint32_t lane = 0; lane < MBLS_CMT_STEP; lane++) if (cms_listed(words, o, base + lane, m, comp)) ballot |= 1ull << lane;
            for (uint32_t lane = 0; lane < MBLS_CMT_STEP; lane++)
                if ((ballot >> lane) & 1ull) {
                    const uint32_t v = members ? members[(uint64_t)firsts[t] + base + lane] : o + base + lane;
                    region[comp ? cms_missing_pos(stride, n_missing, ballot, lane) : cms_direct_pos(n_direct, ballot, lane)] = v;
                }
            if (comp) n_missing += cmt_popcount(ballot); else n_direct += cmt_popcount(ballot);
        }
        if (comp) mask |= 1ull << t;
        total += s; o += m;
    }
    rec[0] = n_direct; rec[1] = n_missing; rec[2] = (uint32_t)mask; rec[3] = (uint32_t)(mask >> 32); rec[4] = total == 0 ? MBLS_CMS_FL_NOBODY : 0u;
}
// the record a malformed item gets: the one index MBLS_CMT_NO_COMMITTEE on the direct list, nothing else (the key sum treats it as any index outside the key table)
MBLS_CFN void cms_reject_item(uint32_t* region, uint32_t* rec) {
    region[0] = MBLS_CMT_NO_COMMITTEE;
    rec[0] = 1u; rec[1] = 0u; rec[2] = 0u; rec[3] = 0u; rec[4] = 0u;
}
// The decision alone, for mbls_plan_committee_span: 0 and the three figures, or -1 for q > 64, a size of 0 or above MBLS_CMT_MAX_MEMBERS, a field that does not
// cover the item, or a mode outside 0..2. `bits`: bytes, any alignment (read bytewise: the same bits the kernel reads as words).
static inline int cms_plan_item(const uint32_t* sizes, const uint8_t* eligible, uint32_t q, const uint8_t* bits, uint32_t bits_bytes, int mode,
                                uint64_t* complement_mask, uint32_t* n_direct_listed, uint32_t* n_missing_listed) {
    if (q > MBLS_CMS_MAX_COMMITTEES || mode < 0 || mode > 2) return -1;
    uint64_t M = 0;
    for (uint32_t t = 0; t < q; t++) { if (sizes[t] == 0 || sizes[t] > MBLS_CMT_MAX_MEMBERS) return -1; M += sizes[t]; }
    if (!cms_field_ok(M, bits_bytes)) return -1;
    uint64_t mask = 0; uint32_t nd = 0, nm = 0, o = 0;
    for (uint32_t t = 0; t < q; t++) {
        uint32_t s = 0;
        for (uint32_t j = 0; j < sizes[t]; j++) { const uint32_t p = o + j; s += (bits[p >> 3] >> (p & 7u)) & 1u; }
        if (cms_route(sizes[t], s, eligible[t] != 0, mode)) { mask |= 1ull << t; nm += sizes[t] - s; } else nd += s;
        o += sizes[t];
    }
    *complement_mask = mask; *n_direct_listed = nd; *n_missing_listed = nm;
    return 0;
}
#endif

// mbls_cmt_lanes.h -- the device bodies of the committee table's kernels (include/mbls.h, "committee table"; the arithmetic they run is mbls_cmt.h):
//   wave_cmt_expand     one WAVE per item: committee + bitfield -> the item's index list, count and route       (k_cmt_expand)
//   lane_aggregate_cmt  one lane per item: the indexed key sum over that list, the complement's fix-up, status  (k_aggregate_cmt_d)
//   lane_cmt_build      one lane per appended committee: key sum + status of the append -> the committee record  (k_cmt_build)
//   lane_cmt_export     the cached sum of one committee as 96 uncompressed bytes                                 (k_cmt_export)
//   wave_vmc_expand     one WAVE per set of a verify_multiple call: committee set or single-key set (mbls_vmc.h)  (k_vmc_expand)
#pragma once
#include "mbls_ops.h"
#include "mbls_cmt.h"
#include "mbls_vmc.h"

// the per-item words k_cmt_expand leaves for k_aggregate_cmt_d beside the list: cnt[i] entries listed; route[i] bit 0 complement, bit 1 nobody selected
#define MBLS_CMT_RT_COMPLEMENT 1u
#define MBLS_CMT_RT_NOBODY 2u

// Item i on the 64 lanes of one wave. The committee's members are walked 64 per step: lane l looks at member base + l, the listed lanes are balloted and each
// writes its member's key index at the position mbcnt gives it -- the member array is read and the list written in runs of consecutive dwords. The bitfield is
// read as 32-bit words (4-byte aligned, stride a multiple of 4, 8 * stride >= the committee's size: checked by the entries). list_stride >= 1 entries per item.
// A committee id that names nothing lists the one index MBLS_CMT_NO_COMMITTEE on the direct route: the key sum treats it as any index outside the key table.
MBLS_FN void wave_cmt_expand(uint64_t i, uint32_t lane, const uint32_t* crecs, uint64_t ccount, const uint32_t* members, const uint32_t* cmt_idx, const uint8_t* bits,
                             uint32_t bits_stride, int mode, uint32_t* list, uint64_t list_stride, uint32_t* cnt, uint32_t* route) {
    uint32_t* out_list = list + list_stride * i;
    const uint32_t cid = cmt_idx[i];
    if ((uint64_t)cid >= ccount) {
        if (lane == 0) { out_list[0] = MBLS_CMT_NO_COMMITTEE; cnt[i] = 1u; route[i] = 0u; }
        return;
    }
    const uint32_t* rec = crecs + (uint64_t)MBLS_CMT_REC_DWORDS * cid;
    const uint32_t first = rec[0], m = rec[1], eligible = rec[2];
    const uint32_t* words = (const uint32_t*)(bits + (uint64_t)bits_stride * i);
    // s: every lane counts the words itself (at most 64 of them, the same addresses on every lane: one broadcast load each)
    const uint32_t s = cmt_count_selected(words, m);
    const int comp = cmt_route(m, s, (int)eligible, mode);
    uint32_t out = 0;
    for (uint32_t base = 0; base < m; base += MBLS_CMT_STEP) {
        const uint32_t j = base + lane;
        const bool want = cmt_listed(words, j, m, comp) != 0;
        const uint64_t ballot = __ballot(want);
        if (want) out_list[cmt_pos(out, ballot, lane)] = members[(uint64_t)first + j];
        out += cmt_popcount(ballot);
    }
    if (lane == 0) { cnt[i] = out; route[i] = (comp ? MBLS_CMT_RT_COMPLEMENT : 0u) | (s == 0 ? MBLS_CMT_RT_NOBODY : 0u); }
}

static_assert(MBLS_VMC_RT_COMPLEMENT == MBLS_CMT_RT_COMPLEMENT && MBLS_VMC_RT_NOBODY == MBLS_CMT_RT_NOBODY, "mbls_vmc.h restates the route word");
// Set i of a verify_multiple call over committees (mbls_vmc.h): a single-key set lists its one key index on the direct route and never touches its bitfield bytes;
// every other word is an item of the committee entries and runs wave_cmt_expand, unchanged (a bit-31-clear id at or above the count names no committee there).
MBLS_FN void wave_vmc_expand(uint64_t i, uint32_t lane, const uint32_t* crecs, uint64_t ccount, const uint32_t* members, const uint32_t* cmt_idx, const uint8_t* bits,
                             uint32_t bits_stride, int mode, uint32_t* list, uint64_t list_stride, uint32_t* cnt, uint32_t* route) {
    const uint32_t word = cmt_idx[i];
    if (vmc_is_single(word)) {
        if (lane == 0) { list[list_stride * i] = vmc_key_index(word); cnt[i] = vmc_single_count(); route[i] = vmc_single_route(); }
        return;
    }
    wave_cmt_expand(i, lane, crecs, ccount, members, cmt_idx, bits, bits_stride, mode, list, list_stride, cnt, route);
}

#if MBLS_DEVICE_ASM && !defined(MBLS_NO_FP2_ASM)
// Item i's key sum from its list: lane_aggregate_d<true>, unchanged, sums the listed keys into the APK slots (MBLS_MODE_VERIFY: the NO_KEYS and APK_INFINITY
// verdicts are formed here, from the route word and the FINAL point). On a complement item the listed keys are the missing members: the final point is the
// committee's cached sum plus the negated list sum, by the compiled group law (g1_add: equal operands double -- the missing sum equals its own negative's
// partner --, opposite operands give infinity -- the missing sum equals the full sum --, and an infinite operand -- the empty list -- leaves the other).
MBLS_FN uint32_t lane_aggregate_cmt(const mbls_ws& ws, uint64_t i, uint32_t lane, const uint32_t* recs, uint64_t tsize, const uint32_t* list, uint64_t list_stride,
                                    const uint32_t* cnt, const uint32_t* route, const uint32_t* crecs, const uint32_t* cmt_idx) {
    const uint32_t c = cnt[i], rt = route[i];
    uint32_t st = lane_aggregate_d<true>(ws, i, list + list_stride * i, c, MBLS_MODE_VERIFY, lane, recs, tsize);
    bool inf;
    if (rt & MBLS_CMT_RT_COMPLEMENT) {
        const uint32_t* rec = crecs + (uint64_t)MBLS_CMT_REC_DWORDS * cmt_idx[i] + MBLS_CMT_REC_SUM;
        g1j full, miss;
#pragma unroll
        for (int t = 0; t < 12; t++) { full.x[t] = rec[t]; full.y[t] = rec[12 + t]; full.z[t] = rec[24 + t]; }
        miss.x = ws_ld(ws, MBLS_SLOT_APK, i); miss.y = ws_ld(ws, MBLS_SLOT_APK + 1, i); miss.z = ws_ld(ws, MBLS_SLOT_APK + 2, i);
        g1_neg(&miss, &miss);
        g1j acc; g1_add(&acc, &full, &miss);
        ws_st(ws, MBLS_SLOT_APK, i, acc.x); ws_st(ws, MBLS_SLOT_APK + 1, i, acc.y); ws_st(ws, MBLS_SLOT_APK + 2, i, acc.z);
        inf = g1_is_inf(&acc);
    } else
        inf = fp_is_zero(ws_ld(ws, MBLS_SLOT_APK + 2, i));
    if (rt & MBLS_CMT_RT_NOBODY) st |= MBLS_ST_NO_KEYS;
    if (inf) st |= MBLS_ST_APK_INFINITY;
    return st;
}
#endif

// committee c of an append: the sum k_aggregate_indexed_d left in workspace item c and the status bits it reported become the record
MBLS_FN void lane_cmt_build(const mbls_ws& ws, uint64_t c, const uint32_t* st, const uint32_t* offsets, uint64_t member_base, uint32_t* crecs) {
    uint32_t* rec = crecs + (uint64_t)MBLS_CMT_REC_DWORDS * c;
    const fp x = ws_ld(ws, MBLS_SLOT_APK, c), y = ws_ld(ws, MBLS_SLOT_APK + 1, c), z = ws_ld(ws, MBLS_SLOT_APK + 2, c);
    rec[0] = (uint32_t)(member_base + offsets[c]); rec[1] = offsets[c + 1] - offsets[c];
    rec[2] = (st[c] & (MBLS_ST_BAD_PK_ENCODING | MBLS_ST_PK_INFINITY)) ? 0u : 1u; rec[3] = 0u;
#pragma unroll
    for (int t = 0; t < 12; t++) { rec[MBLS_CMT_REC_SUM + t] = x[t]; rec[MBLS_CMT_REC_SUM + 12 + t] = y[t]; rec[MBLS_CMT_REC_SUM + 24 + t] = z[t]; }
}
MBLS_FN void lane_cmt_export(const uint32_t* rec, uint8_t* out96) {
    g1j a;
#pragma unroll
    for (int t = 0; t < 12; t++) { a.x[t] = rec[MBLS_CMT_REC_SUM + t]; a.y[t] = rec[MBLS_CMT_REC_SUM + 12 + t]; a.z[t] = rec[MBLS_CMT_REC_SUM + 24 + t]; }
    fp x, y; bool inf; g1_to_affine(&x, &y, &inf, &a); g1_encode_uncompressed(out96, x, y, inf);
}

// mbls_cms_lanes.h -- the device bodies of the committee-span kernels (include/mbls.h, "committee spans"; the arithmetic they run is mbls_cms.h):
//   wave_cms_expand     one WAVE per item: committee list + concatenated bitfield -> the item's direct list, missing list and record   (k_cms_expand)
//   lane_aggregate_cms  one lane per item: missing-list sum, the cached sums' fix-up, the parked point, direct-list sum, status        (k_aggregate_cms_d)
#pragma once
#include "mbls_ops.h"
#include "mbls_cms.h"

// Item i on the 64 lanes of one wave. Everything that decides the control flow is the same on every lane (the offsets, the ids, the records and the counts are
// broadcast loads), so every ballot sees the whole wave. The item's shape is checked BEFORE anything it names is read: the offsets before the ids, the ids before
// the records, the total M before the field. A malformed item lists the one index MBLS_CMT_NO_COMMITTEE (cms_reject_item). The segments are then walked in order,
// each like an item of wave_cmt_expand at its bit offset: 64 members per step, positions from ballot and mbcnt, the selected members of a direct segment to the
// front of the item's region, the missing members of a complement segment to its back. The field is read as 32-bit words (4-byte aligned, the stride a multiple
// of 4, M <= 8 * bits_stride: no word past the item's field is touched); stride >= max(M, 1) words per item (cms_stride).
MBLS_FN void wave_cms_expand(uint64_t i, uint32_t lane, const uint32_t* crecs, uint64_t ccount, const uint32_t* members, const uint32_t* cmt_ids, uint64_t n_cmt_ids,
                             const uint32_t* cmt_off, const uint8_t* bits, uint32_t bits_stride, int mode, uint32_t* list, uint64_t stride, uint32_t* item_recs) {
    uint32_t* region = list + stride * i;
    uint32_t* rec = item_recs + (uint64_t)MBLS_CMS_REC_DWORDS * i;
    const uint32_t off_lo = cmt_off[i], off_hi = cmt_off[i + 1];
    uint32_t q = 0;
    bool ok = cms_range_ok(off_lo, off_hi, n_cmt_ids, &q) != 0;
    uint64_t M = 0;
    if (ok)
        for (uint32_t t = 0; t < q; t++) {
            const uint32_t cid = cmt_ids[(uint64_t)off_lo + t];
            if ((uint64_t)cid >= ccount) { ok = false; break; }
            M += crecs[(uint64_t)MBLS_CMT_REC_DWORDS * cid + 1];
        }
    if (ok) ok = cms_field_ok(M, bits_stride) != 0;
    if (!ok) {
        if (lane == 0) cms_reject_item(region, rec);
        return;
    }
    const uint32_t* words = (const uint32_t*)(bits + (uint64_t)bits_stride * i);
    uint32_t o = 0, n_direct = 0, n_missing = 0, total = 0;
    uint64_t mask = 0;
    for (uint32_t t = 0; t < q; t++) {
        const uint32_t* crec = crecs + (uint64_t)MBLS_CMT_REC_DWORDS * cmt_ids[(uint64_t)off_lo + t];
        const uint32_t first = crec[0], m = crec[1], eligible = crec[2];
        // s: every lane counts the segment's words itself (the same addresses on every lane: one broadcast load each)
        const uint32_t s = cms_count_selected(words, o, m);
        const int comp = cms_route(m, s, (int)eligible, mode);
        for (uint32_t base = 0; base < m; base += MBLS_CMT_STEP) {
            const uint32_t j = base + lane;
            const bool want = cms_listed(words, o, j, m, comp) != 0;
            const uint64_t ballot = __ballot(want);
            if (want) region[comp ? cms_missing_pos(stride, n_missing, ballot, lane) : cms_direct_pos(n_direct, ballot, lane)] = members[(uint64_t)first + j];
            if (comp) n_missing += cmt_popcount(ballot); else n_direct += cmt_popcount(ballot);
        }
        if (comp) mask |= 1ull << t;
        total += s; o += m;
    }
    if (lane == 0) {
        rec[0] = n_direct; rec[1] = n_missing; rec[2] = (uint32_t)mask; rec[3] = (uint32_t)(mask >> 32); rec[4] = total == 0 ? MBLS_CMS_FL_NOBODY : 0u;
    }
}

#if MBLS_DEVICE_ASM && !defined(MBLS_NO_FP2_ASM)
// Item i's key sum from its two lists and its record, with lane_aggregate_d<true> unchanged (MBLS_MODE_VERIFY: NO_KEYS and APK_INFINITY are formed here, from the
// record and the FINAL point):
//   1. the missing list's sum into the APK slots -- only where some lane of the wave has a complement segment (a wave-uniform test; lanes without one sum nothing);
//   2. that sum negated, plus the cached sum of every masked segment's committee by the compiled group law (g1_add: equal operands double -- the same id twice --,
//      opposite operands give infinity -- two committees whose sums cancel, or everybody missing --, an infinite operand leaves the other);
//   3. parked in the context's span scratch (park: [MBLS_CMS_PARK_DWORDS][park_stride] words, item i at column i), not in the workspace and not in registers: the
//      generated routine below owns every register;
//   4. the direct list's sum into the APK slots, plus the parked point.
// The missing members belong to eligible committees (valid, finite table entries): their sum reports no status bit, so the bits are the direct list's alone.
MBLS_FN uint32_t lane_aggregate_cms(const mbls_ws& ws, uint64_t i, uint32_t lane, const uint32_t* recs, uint64_t tsize, const uint32_t* list, uint64_t stride,
                                    const uint32_t* item_recs, const uint32_t* crecs, const uint32_t* cmt_ids, const uint32_t* cmt_off, uint32_t* park,
                                    uint64_t park_stride) {
    const uint32_t* rec = item_recs + (uint64_t)MBLS_CMS_REC_DWORDS * i;
    const uint32_t* region = list + stride * i;
    const uint32_t n_direct = rec[0], n_missing = rec[1], fl = rec[4];
    const uint64_t mask = (uint64_t)rec[2] | ((uint64_t)rec[3] << 32);
    if (__ballot(mask != 0)) {
        (void)lane_aggregate_d<true>(ws, i, region + (n_missing ? cms_missing_first(stride, n_missing) : 0u), n_missing, MBLS_MODE_VERIFY, lane, recs, tsize);
        if (mask) {
            g1j acc; acc.x = ws_ld(ws, MBLS_SLOT_APK, i); acc.y = ws_ld(ws, MBLS_SLOT_APK + 1, i); acc.z = ws_ld(ws, MBLS_SLOT_APK + 2, i);
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
#pragma unroll
            for (int u = 0; u < 12; u++) { park[(uint64_t)u * park_stride + i] = acc.x[u]; park[(uint64_t)(12 + u) * park_stride + i] = acc.y[u]; park[(uint64_t)(24 + u) * park_stride + i] = acc.z[u]; }
        }
    }
    uint32_t st = lane_aggregate_d<true>(ws, i, region, n_direct, MBLS_MODE_VERIFY, lane, recs, tsize);
    bool inf;
    if (mask) {
        g1j parked, acc;
#pragma unroll
        for (int u = 0; u < 12; u++) { parked.x[u] = park[(uint64_t)u * park_stride + i]; parked.y[u] = park[(uint64_t)(12 + u) * park_stride + i]; parked.z[u] = park[(uint64_t)(24 + u) * park_stride + i]; }
        acc.x = ws_ld(ws, MBLS_SLOT_APK, i); acc.y = ws_ld(ws, MBLS_SLOT_APK + 1, i); acc.z = ws_ld(ws, MBLS_SLOT_APK + 2, i);
        g1_add(&acc, &acc, &parked);
        ws_st(ws, MBLS_SLOT_APK, i, acc.x); ws_st(ws, MBLS_SLOT_APK + 1, i, acc.y); ws_st(ws, MBLS_SLOT_APK + 2, i, acc.z);
        inf = g1_is_inf(&acc);
    } else
        inf = fp_is_zero(ws_ld(ws, MBLS_SLOT_APK + 2, i));
    if (fl & MBLS_CMS_FL_NOBODY) st |= MBLS_ST_NO_KEYS;
    if (inf) st |= MBLS_ST_APK_INFINITY;
    return st;
}
#endif

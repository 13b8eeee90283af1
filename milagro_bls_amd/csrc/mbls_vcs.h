// mbls_vcs.h -- verify_multiple over committee SPANS (include/mbls.h, mbls_verify_multiple_committee_span_msgtable*): the set descriptor, the host statement of
// the expansion k_vcs_expand runs, and the rule that cuts a set's two key lists into chunks for lanes of their own. A header of its own in the host-and-device
// style of mbls_vmc.h and mbls_cms.h, so that a host compiler can build it for the CPU tests (tests/vcs_emul/mbls_vcs_harness.cpp).
//
// A set is an item of the span entries (mbls_cms.h): the ids cmt_ids[cmt_off[i] .. cmt_off[i + 1]) and one field over the concatenated members, every rule
// unchanged. ONE more kind of set rides along, as in mbls_vmc.h: a set of EXACTLY ONE id with bit 31 set (MBLS_VM_SET_SINGLE_KEY | key index) is a set under one
// validator key -- its list is that one index on the direct route, its field bytes are not read, an index outside the key table rejects the set through the key sum.
// A bit-31 id among two or more ids names no committee (no table holds 2^31 committees): the set is malformed like any set with an id at or above the count.
//
// THE SPLIT. The span key sum (lane_aggregate_cms) gives one lane per item, which is right for the thousands of items of fast_aggregate_verify. A block's
// verify_multiple call is about a dozen sets: one lane then walks a chain of up to 8 192 additions while the rest of the chip idles. With split factor P > 1 each
// of a set's two lists is cut into P chunks, chunk p of a list of L entries being [floor(p L / P), floor((p + 1) L / P)) -- the chunks tile [0, L), an empty one
// leaves infinity --, every chunk is summed by a lane of its own (k_vcs_partial_d: lane g = (2 i + list) P + p, list 0 the missing list, list 1 the direct list, so
// a set's chunks sit in adjacent lanes) into workspace item base + g, and one lane per set adds the partial sums up (k_vcs_combine).
#ifndef MBLS_VCS_H
#define MBLS_VCS_H
#include "../../include/mbls.h"
#include "mbls_cms.h"
#include "mbls_vmc.h"

#define MBLS_VCS_MAX_SPLIT 16u
// THE AUTO RULE (mode 0), settled by profiles/vm_committee_span_throughput.json. A split is taken while the call has at most
// MBLS_VCS_SPLIT_MAX_SETS sets (the largest call measured: 4 096 sets at 45 % take 13.6 ms with P = 4 against 43.2 with P = 1) and the chunks' lanes fill at most
// HALF a round (4 P n <= round_items: at 4 096 sets P = 8, a full round of lanes, is no faster than P = 4). A chunk is worth a lane when the region -- the bound on
// a list's length the host knows, cms_stride -- gives it at least MBLS_VCS_MIN_CHUNK entries (chunks of 10 entries still pay, chunks of 5 do not: a block's 82
// absentees at 99 % take 5.13, 5.16 and 5.26 ms with P = 4, 8 and 16).
#define MBLS_VCS_SPLIT_MAX_SETS 4096u
#define MBLS_VCS_MIN_CHUNK 8u

// ---- the descriptor
// is the set [off_lo, off_hi) a single-key set: exactly one id, bit 31 set (the caller has checked the range and reads ids[off_lo] only when q == 1)
MBLS_CFN int vcs_is_single(uint32_t q, uint32_t first_id) { return q == 1u && vmc_is_single(first_id); }
// does an id of a set that is NOT single-key name a committee: bit 31 never does
MBLS_CFN int vcs_id_ok(uint32_t id, uint64_t ccount) { return !vmc_is_single(id) && (uint64_t)id < ccount; }
// what the host entries refuse beside the malformed kinds: a single-key index that names no key
MBLS_CFN int vcs_single_names_nothing(uint32_t id, uint64_t tsize) { return (uint64_t)vmc_key_index(id) >= tsize; }
// the record and the region of a single-key set: one entry on the direct list, no missing entry, no masked segment, somebody selected
MBLS_CFN void vcs_single_item(uint32_t id, uint32_t* region, uint32_t* rec) {
    region[0] = vmc_key_index(id);
    rec[0] = 1u; rec[1] = 0u; rec[2] = 0u; rec[3] = 0u; rec[4] = 0u;
}
// The whole expansion of one set as the wave runs it (the host statement of k_vcs_expand), in the span section's read order: offsets, ids, records, M, field.
// crecs: the committee records (MBLS_CMT_REC_DWORDS words each, ccount of them: [0] first member, [1] size, [2] eligible), members: the member array, words: the
// set's field. region: `stride` words, rec: MBLS_CMS_REC_DWORDS. Returns 0 single-key, 1 expanded, 2 rejected (malformed).
MBLS_CFN int vcs_expand_set(uint32_t off_lo, uint32_t off_hi, const uint32_t* cmt_ids, uint64_t n_cmt_ids, const uint32_t* crecs, uint64_t ccount, const uint32_t* members,
                            const uint32_t* words, uint32_t bits_stride, int mode, uint32_t* region, uint64_t stride, uint32_t* rec) {
    uint32_t q = 0;
    if (!cms_range_ok(off_lo, off_hi, n_cmt_ids, &q)) { cms_reject_item(region, rec); return 2; }
    if (q == 1u && vcs_is_single(q, cmt_ids[off_lo])) { vcs_single_item(cmt_ids[off_lo], region, rec); return 0; }
    uint32_t sizes[MBLS_CMS_MAX_COMMITTEES], firsts[MBLS_CMS_MAX_COMMITTEES]; uint8_t eligible[MBLS_CMS_MAX_COMMITTEES];
    uint64_t M = 0;
    for (uint32_t t = 0; t < q; t++) {
        const uint32_t id = cmt_ids[(uint64_t)off_lo + t];
        if (!vcs_id_ok(id, ccount)) { cms_reject_item(region, rec); return 2; }
        const uint32_t* cr = crecs + (uint64_t)MBLS_CMT_REC_DWORDS * id;
        firsts[t] = cr[0]; sizes[t] = cr[1]; eligible[t] = (uint8_t)(cr[2] != 0u);
        M += cr[1];
    }
    if (!cms_field_ok(M, bits_stride)) { cms_reject_item(region, rec); return 2; }
    cms_expand_item(words, members, sizes, firsts, eligible, q, mode, region, stride, rec);
    return 1;
}

// ---- the split
MBLS_CFN int vcs_split_mode_ok(int mode) { return mode == 0 || mode == 1 || mode == 2 || mode == 4 || mode == 8 || mode == 16; }
// chunk p of a list of L entries under split factor P: [vcs_chunk_lo(L, P, p), vcs_chunk_lo(L, P, p + 1))
MBLS_CFN uint32_t vcs_chunk_lo(uint32_t L, uint32_t P, uint32_t p) { return (uint32_t)(((uint64_t)p * L) / P); }
// lane g of k_vcs_partial_d: its set, its list (0 missing, 1 direct) and its chunk; and back
MBLS_CFN uint64_t vcs_lane_set(uint64_t g, uint32_t P) { return g / (2u * P); }
MBLS_CFN uint32_t vcs_lane_list(uint64_t g, uint32_t P) { return (uint32_t)((g % (2u * P)) / P); }
MBLS_CFN uint32_t vcs_lane_chunk(uint64_t g, uint32_t P) { return (uint32_t)(g % P); }
MBLS_CFN uint64_t vcs_lane_of(uint64_t i, uint32_t list, uint32_t p, uint32_t P) { return (2u * i + list) * P + p; }
// the workspace items a call takes behind what the message-table entries plan: the partial sums, none without a split
MBLS_CFN uint64_t vcs_extra_items(uint64_t n, uint32_t P) { return P > 1u ? 2u * (uint64_t)P * n : 0u; }
// The split factor of a call of n sets whose regions take `stride` words (cms_stride). mode: mbls_ctx_set_vm_span_split's -- 0 auto, else the factor asked for.
// Whatever the mode, 2 P n never exceeds a round (every chunk has its lane in ONE launch at one wave per SIMD; P is halved until that holds: P = 1 always does),
// and auto answers 1 once 2 n reaches a round, where verify_multiple_impl stops running its chains side by side. Auto takes the largest factor whose lanes fill at
// most half a round and that leaves every chunk of a full region at least MBLS_VCS_MIN_CHUNK entries.
MBLS_CFN uint32_t vcs_split(uint64_t n, uint64_t stride, const mbls_limits* limits, int mode) {
    if (!vcs_split_mode_ok(mode) || n == 0) return 1u;
    const uint64_t R = limits->round_items;
    uint32_t P = mode ? (uint32_t)mode : MBLS_VCS_MAX_SPLIT;
    if (!mode && (2u * n >= R || n > MBLS_VCS_SPLIT_MAX_SETS)) return 1u;
    while (P > 1u && (2u * (uint64_t)P * n > R || (!mode && (4u * (uint64_t)P * n > R || stride < (uint64_t)P * MBLS_VCS_MIN_CHUNK)))) P /= 2u;
    return P;
}
#endif

// mbls_vmc.h -- the set descriptor of mbls_verify_multiple_committee_msgtable* (include/mbls.h, "verify_multiple over committee bitfields"): what one uint32 of
// cmt_idx names, and what a set's key list, count and route words are. A header of its own, like mbls_cmt.h and mbls_vmt.h, so that a host compiler can build it for
// the CPU tests (tests/vmc_emul/mbls_vmc_harness.cpp): k_vmc_expand of mbls_kernels.hip runs exactly vmc_is_single, vmc_key_index and -- for a committee set --
// the expansion of mbls_cmt.h, unchanged.
//
// A gossip batch mixes two kinds of set. A COMMITTEE set (bit 31 of the word clear) is an item of the committee entries: the word is a committee id, the set's
// bits_stride bytes are its SSZ bitfield, every rule is mbls_cmt.h's (bits at or above the committee's size ignored, route by cmt_route, an id at or above the count
// lists the one index MBLS_CMT_NO_COMMITTEE). A SINGLE-KEY set (bit 31 set: MBLS_VM_SET_SINGLE_KEY) is a selection proof, an aggregator's signature or an
// unaggregated attestation: the low 31 bits are an index into the key table the committee table is bound to, the set's list is that one index on the direct route,
// and its bitfield bytes are NOT READ. An index outside the key table rejects the set through the key sum like any other (0xFFFFFFFF names key 0x7FFFFFFF, which
// no table holds: it still rejects).
#ifndef MBLS_VMC_H
#define MBLS_VMC_H
#include "mbls_cmt.h"

#define MBLS_VMC_SINGLE_KEY 0x80000000u       // include/mbls.h MBLS_VM_SET_SINGLE_KEY
// the route word of a set (mbls_cmt_lanes.h MBLS_CMT_RT_*, restated for the host build): bit 0 complement, bit 1 nobody selected
#define MBLS_VMC_RT_COMPLEMENT 1u
#define MBLS_VMC_RT_NOBODY 2u
// The status bits the key phase of verify_multiple reports per set: those of the indexed key sum under verify_multiple (an undecodable or missing member, a member
// at infinity). The empty list and the sum at infinity are NOT verdicts of verify_multiple's key phase -- the indexed entries report neither, an infinite key walks
// its Miller loop and contributes 1 --, so k_aggregate_vmc_d drops the two bits lane_aggregate_cmt forms for the fast_aggregate_verify entries.
#define MBLS_VMC_KEY_STATUS_MASK (~(0x08u /* MBLS_ST_APK_INFINITY */ | 0x10u /* MBLS_ST_NO_KEYS */))

MBLS_CFN int vmc_is_single(uint32_t word) { return (word & MBLS_VMC_SINGLE_KEY) != 0u; }
// the key-table index a single-key set names (the caller has checked vmc_is_single)
MBLS_CFN uint32_t vmc_key_index(uint32_t word) { return word & ~MBLS_VMC_SINGLE_KEY; }
// a single-key set's words: the list is {vmc_key_index(word)}, one entry, direct route, somebody selected
MBLS_CFN uint32_t vmc_single_count(void) { return 1u; }
MBLS_CFN uint32_t vmc_single_route(void) { return 0u; }
// the route word of a committee set from what the expansion found
MBLS_CFN uint32_t vmc_route_word(int complement, uint32_t selected) { return (complement ? MBLS_VMC_RT_COMPLEMENT : 0u) | (selected == 0u ? MBLS_VMC_RT_NOBODY : 0u); }
MBLS_CFN uint32_t vmc_key_status(uint32_t st) { return st & MBLS_VMC_KEY_STATUS_MASK; }
// does the host refuse the word: a committee id at or above the count, a single-key index at or above the key table's size
MBLS_CFN int vmc_names_nothing(uint32_t word, uint64_t ccount, uint64_t tsize) {
    return vmc_is_single(word) ? (uint64_t)vmc_key_index(word) >= tsize : (uint64_t)word >= ccount;
}
// The whole expansion of one set as the wave runs it (the host statement of k_vmc_expand). crecs: the committee records (MBLS_CMT_REC_DWORDS words each, ccount of
// them), members: the member array, words: the set's bitfield. list: room for max(1, largest committee) entries. Returns the count; *route receives the route word.
MBLS_CFN uint32_t vmc_expand_set(uint32_t word, const uint32_t* crecs, uint64_t ccount, const uint32_t* members, const uint32_t* words, int mode, uint32_t* list,
                                 uint32_t* route) {
    if (vmc_is_single(word)) { list[0] = vmc_key_index(word); *route = vmc_single_route(); return vmc_single_count(); }
    if ((uint64_t)word >= ccount) { list[0] = MBLS_CMT_NO_COMMITTEE; *route = 0u; return 1u; }
    const uint32_t* rec = crecs + (uint64_t)MBLS_CMT_REC_DWORDS * word;
    const uint32_t first = rec[0], m = rec[1], eligible = rec[2];
    int comp = 0;
    const uint32_t out = cmt_expand_item(words, members + first, m, (int)eligible, mode, list, &comp);
    *route = vmc_route_word(comp, cmt_count_selected(words, m));
    return out;
}
#endif

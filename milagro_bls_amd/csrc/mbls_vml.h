// mbls_vml.h -- the pure rules of mbls_verify_multiple_batches_locate* (include/mbls.h, "WHICH SETS OF A REJECTED BATCH"): what one set of a call becomes once
// its batch's verdict is known -- answered at once or a candidate for a pairing check of its own -- and where the sets' shadow items lie in the workspace.
// A header of its own, like mbls_vmb.h, so that a host compiler can build it for the CPU tests (tests/vml_emul/mbls_vml_harness.cpp); k_vml_mark of
// mbls_kernels.hip runs exactly vml_mark, and vmb_impl reserves exactly vml_workspace_items.
#ifndef MBLS_VML_H
#define MBLS_VML_H
#include "mbls_vmb.h"

// the bits that reject a verify_multiple batch (mbls_coop.h COOP_REJECT_BATCH, mbls_lanes.h final_fold_batch; values of include/mbls.h): a set carrying one of
// them in its own word is rejected as the one-set batch would be, without a pairing
#define MBLS_VML_REJECT (0x01u /* BAD_SIG_ENCODING */ | 0x02u /* SIG_NOT_IN_G2 */ | 0x04u /* BAD_PK_ENCODING */ | 0x100u /* BAD_MSG_RANGE */ | 0x80u /* BAD_SCALAR */)
#define MBLS_VML_TABLE_FAULT 0x04u            // MBLS_ST_BAD_PK_ENCODING: the bit mbls_verify_multiple_batches* uses for faults of a device-side batch table

#define MBLS_VML_FALSE 0u                     // vml_mark: the set's answer is 0, no pairing
#define MBLS_VML_TRUE 1u                      //           the set's answer is 1, no pairing
#define MBLS_VML_CANDIDATE 2u                 //           the set's own pairing check decides (phase two)

// One set, after the per-batch tail. owned: a batch with a sound range owns the set and owns every set of that range alone (vmb_owner_range, vmb_owns_all);
// batch_ok: that batch's result byte; st: the set's own status word as phase one left it. *st_out: the word the call reports for the set before phase two
// (phase two adds MBLS_ST_PAIRING_FAILED to a candidate whose check fails).
//   no owner          -> 0, with the table-fault bit: the set is part of no batch the call could judge
//   accepted batch    -> 1: NOT examined (the batch check is the security statement)
//   a rejecting bit   -> 0: what the one-set batch answers without a pairing
//   otherwise         -> candidate
MBLS_VFN uint32_t vml_mark(bool owned, bool batch_ok, uint32_t st, uint32_t* st_out) {
    *st_out = owned ? st : (st | MBLS_VML_TABLE_FAULT);
    if (!owned) return MBLS_VML_FALSE;
    if (batch_ok) return MBLS_VML_TRUE;
    if (st & MBLS_VML_REJECT) return MBLS_VML_FALSE;
    return MBLS_VML_CANDIDATE;
}
// the first shadow item: behind everything phase one works on (mbls_vmb.h vmb_workspace_items -- the lane-pair message phase's 2 n items included, which
// runs beside the signature chain that fills the shadows)
MBLS_VFN uint64_t vml_shadow_first(uint64_t n, uint64_t B, bool pair_hash) { return vmb_workspace_items(n, B, pair_hash); }
// workspace items of a locate call: phase one's, and one shadow item per set -- 2 n + 2 B, or 3 n for calls whose message phase runs on lane pairs
MBLS_VFN uint64_t vml_workspace_items(uint64_t n, uint64_t B, bool pair_hash) { return vml_shadow_first(n, B, pair_hash) + n; }
// status words a locate call keeps in the context: the sets' [0, n), the batches' [n, n + B), the ownership counts [n + B, n + 2 B), the candidate flags
// [n + 2 B, 2 n + 2 B) -- never more than the workspace items, which are 2 n + 2 B or, where 2 n > n + 2 B, 3 n > 2 n + 2 B (the context holds one word per item)
MBLS_VFN uint64_t vml_flags_first(uint64_t n, uint64_t B) { return n + 2 * B; }
#endif

// mbls_vsl.h -- the pure rules of mbls_verify_multiple*_shared_msgs_locate* (include/mbls.h, "WHICH SETS OF A REJECTED SHARED-MESSAGE CALL"): what one set of a
// call over a shared message list becomes once the call's verdict is known, and where the sets' shadow items lie in the workspace. A header of its own, like
// mbls_vml.h and mbls_vms.h, so that a host compiler can build it for the CPU tests (tests/vsl_emul/mbls_vsl_harness.cpp); k_vsl_mark of mbls_kernels.hip runs
// exactly vsl_mark, and verify_multiple_impl reserves exactly vsl_workspace_items.
#ifndef MBLS_VSL_H
#define MBLS_VSL_H
#include "mbls_vml.h"
#include "mbls_vms.h"

#define MBLS_VSL_BAD_MSG 0x100u               // MBLS_ST_BAD_MSG_RANGE: the bit a message fault puts into the word of every set that names the message

// The word of set i as the one-set call with its message spelled out would find it. The grouped route reports a listed message with a bad range in the CALL's
// word only (k_vms_heads), so the set's word gets the bit here, looked up through the set's own index: msg_idx >= n_msgs (n_msgs = 0: every index) names no
// message -- k_vms_count has put the bit there already, and `flags` is not read --, otherwise flags[msg_idx + 1] is the bad-range bit of the listed message
// (entry 0 of the table is the empty message's: lane_h_export, lane_h_gather).
MBLS_VFN uint32_t vsl_own_word(uint32_t st, uint32_t msg_idx, uint64_t n_msgs, const uint32_t* flags) {
    if (vms_group(msg_idx, n_msgs) == MBLS_VMS_NO_GROUP) return st | MBLS_VSL_BAD_MSG;
    return st | (flags[(uint64_t)msg_idx + 1] ? MBLS_VSL_BAD_MSG : 0u);
}
// One set, after the call's tail (grouped route). call_ok: the call's result byte; st: the set's own status word as phase one left it. The answer is
// vml_mark's with the whole call as the one batch that owns every set, on the word vsl_own_word gives:
//   accepted call                     -> 1: NOT examined
//   a rejecting bit, message faults included -> 0, no pairing
//   otherwise                         -> candidate
MBLS_VFN uint32_t vsl_mark(bool call_ok, uint32_t st, uint32_t msg_idx, uint64_t n_msgs, const uint32_t* flags, uint32_t* st_out) {
    return vml_mark(true, call_ok, vsl_own_word(st, msg_idx, n_msgs, flags), st_out);
}
// the shadow items of a set: one on the per-set route (the pair ([r] sig, -G1), and the set's Miller value in slot F: mbls_vml.h's scheme with one batch), two
// on the grouped route, where no Miller value per set exists: A(i) = first + i holds the pair (H(m), [r] apk), B(i) = first + n + i the pair ([r] sig, -G1)
MBLS_VFN uint64_t vsl_shadows_per_set(bool grouped) { return grouped ? 2 : 1; }
// the first shadow item: behind everything phase one works on -- the sets, the Miller items, the positions and the items of the list's own hash
// (mbls_vms.h vms_workspace_items)
MBLS_VFN uint64_t vsl_shadow_first(uint64_t n, uint64_t n_msgs, bool grouped, uint64_t list_workspace_items) {
    return vms_workspace_items(n, n_msgs, grouped, list_workspace_items);
}
MBLS_VFN uint64_t vsl_workspace_items(uint64_t n, uint64_t n_msgs, bool grouped, uint64_t list_workspace_items) {
    return vsl_shadow_first(n, n_msgs, grouped, list_workspace_items) + vsl_shadows_per_set(grouped) * n;
}
// status words a locate call keeps in the context: the sets' [0, n) and the candidate flags [n, 2 n) -- never more than the workspace items (the context
// holds one word per item)
MBLS_VFN uint64_t vsl_flags_first(uint64_t n) { return n; }
// the set a lane of the 2 n-item Miller launch over the shadows answers for: item t of the shadows (A(0..n), then B(0..n)) belongs to set t mod n
MBLS_VFN uint64_t vsl_shadow_set(uint64_t t, uint64_t n) { return t >= n ? t - n : t; }
#endif

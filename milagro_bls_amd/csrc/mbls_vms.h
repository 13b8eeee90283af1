// mbls_vms.h -- the pure grouping arithmetic of mbls_verify_multiple*_shared_msgs (include/mbls.h): n sets in the caller's order, each naming one of n_msgs
// listed messages; the blinded keys of the sets that name message g are moved next to each other -- message g owns the positions [off[g], off[g + 1]), off the
// exclusive scan over the sets-per-message counts -- and summed there by per-message trees (mbls_vmb.h's vmb_takes_partner / vmb_levels), so that the check
// walks one Miller loop per message. Which group a set joins, which position it takes, which range a message owns, what a bad index turns into, and the
// workspace a call needs. A header of its own so that a host compiler can build it for the CPU tests (tests/vms_emul/mbls_vms_harness.cpp); the kernels
// k_vms_count, k_vms_scan, k_vms_scatter, k_g1_seg_tree_d and k_vms_heads of mbls_kernels.hip run exactly these.
#ifndef MBLS_VMS_H
#define MBLS_VMS_H
#include <stdint.h>
#include "mbls_vmb.h"

#define MBLS_VMS_NO_GROUP 0xFFFFFFFFu         // a set whose index names no message of the list joins no group (and rejects the check: MBLS_ST_BAD_MSG_RANGE);
                                              // map[p]: no set stands at position p
#define MBLS_VMS_SCAN_LANES 1024u             // k_vms_scan is ONE workgroup: lane t sums a contiguous chunk of the counts, the chunk sums are scanned in LDS

// the group set i joins: its message, or none for an index outside the list (n_msgs = 0: every index is)
MBLS_VFN uint32_t vms_group(uint32_t msg_idx, uint64_t n_msgs) { return (uint64_t)msg_idx < n_msgs ? msg_idx : MBLS_VMS_NO_GROUP; }
// the chunk of the counts lane t of T walks in the scan: [*lo, *hi), empty beyond the list
MBLS_VFN void vms_scan_chunk(uint64_t n_msgs, uint32_t T, uint32_t t, uint64_t* lo, uint64_t* hi) {
    const uint64_t chunk = (n_msgs + T - 1) / T;
    *lo = chunk * t < n_msgs ? chunk * t : n_msgs;
    *hi = *lo + chunk < n_msgs ? *lo + chunk : n_msgs;
}
// message g's range of positions: off[0 .. n_msgs] is the exclusive scan of the counts, off[n_msgs] = the sets that joined a group at all (<= n)
MBLS_VFN void vms_range(const uint32_t* off, uint64_t g, uint64_t* lo, uint64_t* hi) { *lo = off[g]; *hi = off[g + 1]; }
// The position a set takes: the `ticket`-th arrival of group g (an atomic counter per group hands the tickets out, 0, 1, 2, ... below the group's count) stands
// at off[g] + ticket. WHICH set of a group gets which ticket depends on the order the atomics arrive in and differs from run to run; that every set of the
// group gets exactly one position of the group's range, and every position one set, does not.
MBLS_VFN uint64_t vms_position(const uint32_t* off, uint32_t g, uint32_t ticket) { return (uint64_t)off[g] + ticket; }
// the range position p works in at the tree levels: its message's (through the map position -> message the scatter wrote). false: nobody stands there.
MBLS_VFN bool vms_owner_range(const uint32_t* map, const uint32_t* off, uint64_t n_msgs, uint64_t n, uint64_t p, uint64_t* lo, uint64_t* hi) {
    if (p >= n) return false;
    const uint32_t g = map[p];
    if ((uint64_t)g >= n_msgs) return false;
    vms_range(off, g, lo, hi);
    return *lo <= p && p < *hi && *hi <= n;
}
// routing (mbls_ctx_set_vm_grouping): 1 always one Miller loop per message, 2 never (every set gathers its message's point and walks its own), 0 auto
MBLS_VFN bool vms_grouped(uint64_t n, uint64_t n_msgs, int mode) { return mode == 1 ? true : mode == 2 ? false : 2 * n_msgs <= n; }
// the Miller items of the grouped route: one per listed message (a message no set names gets an infinite key and contributes 1); an empty list still walks
// one item -- infinite key, H of the empty message -- so that the tail finds a product
MBLS_VFN uint64_t vms_miller_items(uint64_t n_msgs) { return n_msgs ? n_msgs : 1; }
// where the positions start in the workspace: behind the sets [0, n) AND behind the Miller items [0, miller_items), whose key slots the heads are written to
// while other groups' positions are still being read
MBLS_VFN uint64_t vms_position_base(uint64_t n, uint64_t n_msgs) { const uint64_t m = vms_miller_items(n_msgs); return n > m ? n : m; }
// workspace items a call needs: grouped -- the sets, the Miller items and the n positions; per set -- the sets; both: the items the list's own hash works in
MBLS_VFN uint64_t vms_workspace_items(uint64_t n, uint64_t n_msgs, bool grouped, uint64_t list_workspace_items) {
    const uint64_t a = grouped ? vms_position_base(n, n_msgs) + n : n;
    return a > list_workspace_items ? a : list_workspace_items;
}
// the tree levels a call enqueues: half = 1, 2, 4, ... < the longest group (the host entries have counted it); a device-side index table: all n sets
MBLS_VFN uint32_t vms_levels(uint64_t n, uint64_t longest_known) { return vmb_levels(longest_known ? longest_known : n); }
#endif

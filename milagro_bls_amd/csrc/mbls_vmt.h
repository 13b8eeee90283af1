// mbls_vmt.h -- the pure arithmetic of mbls_verify_multiple*_msgtable* (include/mbls.h, "verify_multiple over the resident message table"): n sets, each naming
// one of the T entries of a resident message table that outlives the call and may hold far more entries than the call names. The grouping of mbls_vms.h runs
// unchanged with the table as the list (counts, scan, scatter and per-entry sums over T entries); what this header adds is the step from "cnt[j] sets name entry
// j" to the Miller items of the call: the entries that are named at all, compacted in increasing table index (named[0 .. D)), one Miller item per named entry,
// and the sizes the host plans with while D stays on the device. A header of its own, like mbls_vms.h and mbls_mtb.h, so that a host compiler can build it for
// the CPU tests (tests/vmt_emul/mbls_vmt_harness.cpp); k_vmt_flag, k_vmt_named, k_vmt_heads and k_vmt_miller of mbls_kernels.hip, the early exit of k_coop_t and
// plan_vm_msgtable run exactly these.
#ifndef MBLS_VMT_H
#define MBLS_VMT_H
#include <stdint.h>
#include "mbls_vms.h"

#define MBLS_VMT_NO_ENTRY 0xFFFFFFFFu         // the index an idle Miller item reads the table with: it names nothing (mbls_mtb.h mtb_entry: the private entry 0)

// entry j is named when at least one set joined its group (k_vms_count with n_msgs = T); the words are scanned by k_vms_scan like the counts
MBLS_VFN uint32_t vmt_flag(uint32_t cnt) { return cnt != 0 ? 1u : 0u; }
// named[roff[j]] = j for every flagged j: roff[0 .. T] is the exclusive scan of the flags, so the named entries stand in increasing table index and
// roff[T] = D, the number of distinct entries the call names. false: entry j is not named and writes nothing.
MBLS_VFN bool vmt_named_slot(const uint32_t* flag, const uint32_t* roff, uint64_t j, uint32_t* slot) {
    if (!flag[j]) return false;
    *slot = roff[j]; return true;
}
// Miller item r of miller_items. r < D: the pair of table entry named[r] (public index: lane_h_gather maps it to entry + 1) and the sum at the head of its
// range, position off[named[r]]. Otherwise the item is idle: the private entry, the point at infinity (position 0 is read and nothing of it kept).
// false: idle.
MBLS_VFN bool vmt_head(const uint32_t* named, const uint32_t* off, uint64_t D, uint64_t r, uint32_t* idx, uint64_t* pos) {
    if (r >= D) { *idx = MBLS_VMT_NO_ENTRY; *pos = 0; return false; }
    *idx = named[r]; *pos = off[named[r]]; return true;
}
// The bound on D the host sizes the Miller phase with. named_known: D as a host entry has counted it (0: not known -- a device-side index array, never read
// back: at most one entry per set and at most every entry of the table).
MBLS_VFN uint64_t vmt_bound(uint64_t n, uint64_t table_size, uint64_t named_known) { return named_known ? named_known : (n < table_size ? n : table_size); }
// fail closed: a call whose D exceeds the Miller items it was sized with would leave groups out of the product (cannot happen with vmt_bound; checked on the device)
MBLS_VFN bool vmt_overflow(uint64_t D, uint64_t miller_items) { return D > miller_items; }
// routing, Miller items and position base are mbls_vms.h's rules with the bound in place of the list length (vms_grouped, vms_miller_items,
// vms_position_base); so is the workspace, with no list items: nothing is hashed
MBLS_VFN uint64_t vmt_workspace_items(uint64_t n, uint64_t bound, bool grouped) { return vms_workspace_items(n, bound, grouped, 0); }
// the group words a call needs per array (cnt, cur, off, flag, roff: T + 1 each; named: T)
MBLS_VFN uint64_t vmt_group_words(uint64_t table_size) { return table_size + 1; }
// the early exit of the Miller forms: an item index at or above the live count has no pair to walk (live = roff + T on the device). The wave form asks for
// a wave's first item, the lane forms for every lane's item and return when a whole wave has none.
MBLS_VFN bool vmt_wave_idle(uint64_t first_index, uint32_t live) { return first_index >= (uint64_t)live; }
#endif

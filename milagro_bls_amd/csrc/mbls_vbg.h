// mbls_vbg.h -- the pure arithmetic of mbls_verify_multiple_batches_committee_msgtable* (include/mbls.h): B batches over n sets laid out back to back
// (mbls_vmb.h), every set naming one entry of a resident message table. Inside a batch the identity of the shared-message entries holds,
//   prod_i e([r_i] apk_i, H(m_i)) = prod_j e(sum_{i: msg(i) = j} [r_i] apk_i, H(m_j)),
// so a batch needs one Miller loop per DISTINCT entry it names. This header states which sets of a batch form a group, how a batch's groups are numbered, which
// position a set's blinded key moves to, what a Miller item of the grouped route is, the routing rule and the workspace. A header of its own in the style of
// mbls_vmb.h and mbls_vms.h, so that a host compiler can build it for the CPU tests (tests/vbg_emul/mbls_vbg_harness.cpp); the kernels of mbls_vbg.hip and
// plan_vm_batches_committee of mbls_kernels.hip run exactly these.
//
// THE GROUPING (k_vbg_group: one wave per batch, 64 sets per step, over the sets the batch owns under k_vmb_set_map). A set whose index names an entry has a
// LEADER, the lowest set of its batch that names the same entry. A batch's groups are numbered in leader order; a set's rank is the number of earlier sets of its
// group; group g of batch b owns the positions [lo_b + start_b[g], lo_b + start_b[g] + size_b[g]), start_b the exclusive scan of the sizes in group order; a set
// stands at lo_b + start_b[group] + rank. Nothing here depends on the order lanes arrive in: no tickets, every word can be compared with a model.
// A batch's positions and its batch-local group records lie inside its own range [lo_b, hi_b) of the per-set arrays -- a batch has at most as many groups as
// sets --, and a batch writes only there: no word crosses a batch boundary. The positions a batch does not fill (its sets with an index that names nothing)
// are HOLES at the end of its range and keep MBLS_VBG_NONE.
#ifndef MBLS_VBG_H
#define MBLS_VBG_H
#include <stdint.h>
#include "mbls_vmb.h"

#define MBLS_VBG_NONE 0xFFFFFFFFu             // pos[j]: set j stands nowhere; rlo[p] / rhi[p]: nobody stands at position p; head / entry: no such group
// A batch with more sets is not grouped: each of its valid sets is a group of its own (the verdict is the same, the batch walks one Miller loop per set). The
// wave keeps the batch's indices, leaders, ranks, group numbers, sizes and starts in LDS -- 6 words per set, 24 KB at this cap, so that six batches' waves
// fit the 160 KB of a compute unit -- and looks a set's leader up by walking the batch's indices, cap^2 / 64 = 16 384 LDS
// reads per lane at the cap; four times the cap would be 16 times that walk for batches no gossip caller sends (a gossip batch is a few dozen sets).
#define MBLS_VBG_MAX_SETS 1024u
#define MBLS_VBG_WAVE 64u
#define MBLS_VBG_BAD_MSG 0x100u               // MBLS_ST_BAD_MSG_RANGE: the bit of a set whose index names no entry, and of a batch with more groups than the call planned

// does the index name an entry of a table of T entries (T = 0: no index does)
MBLS_VFN bool vbg_valid(uint32_t msg_idx, uint64_t T) { return (uint64_t)msg_idx < T; }
// is a batch of m sets grouped at all
MBLS_VFN bool vbg_batch_grouped(uint64_t m) { return m <= (uint64_t)MBLS_VBG_MAX_SETS; }
// One lane's walk: set j (batch-local) of a batch of m sets whose indices are idx[0 .. m). false: the index names nothing. Otherwise *leader = the lowest set
// naming the same entry (<= j), *rank = the sets of the group in front of j, *size = the sets of the group.
MBLS_VFN bool vbg_lane_walk(const uint32_t* idx, uint32_t m, uint32_t j, uint64_t T, uint32_t* leader, uint32_t* rank, uint32_t* size) {
    const uint32_t mine = idx[j];
    if (!vbg_valid(mine, T)) return false;
    uint32_t l = j, r = 0, s = 0;
    for (uint32_t k = 0; k < m; k++) {
        if (idx[k] != mine) continue;
        s++;
        if (k < j) { r++; if (k < l) l = k; }
    }
    *leader = l; *rank = r; *size = s; return true;
}
// The whole grouping of ONE batch with a sound range [lo, hi) that owns every set of it, as the wave runs it (the host statement of k_vbg_group). msg_idx: the
// call's indices; pos, rlo, rhi, head, entry: the call's per-set arrays, of which only [lo, hi) is written; status: the sets' words. Returns the group count.
MBLS_VFN uint32_t vbg_group_batch(const uint32_t* msg_idx, uint64_t T, uint64_t lo, uint64_t hi, uint32_t* pos, uint32_t* rlo, uint32_t* rhi, uint32_t* head,
                                  uint32_t* entry, uint32_t* status) {
    const uint64_t m = hi - lo;
    uint32_t G = 0;
    if (!vbg_batch_grouped(m)) {      // every valid set a group of its own, in set order
        for (uint64_t j = lo; j < hi; j++) {
            if (!vbg_valid(msg_idx[j], T)) { status[j] |= MBLS_VBG_BAD_MSG; continue; }
            const uint32_t p = (uint32_t)(lo + G);
            pos[j] = p; rlo[p] = p; rhi[p] = p + 1u; head[lo + G] = p; entry[lo + G] = msg_idx[j]; G++;
        }
        return G;
    }
    // leaders in set order give the group numbers and sizes; the exclusive scan of the sizes gives the starts
    uint32_t start = 0;
    for (uint32_t j = 0; j < (uint32_t)m; j++) {
        uint32_t l, r, s;
        if (!vbg_lane_walk(msg_idx + lo, (uint32_t)m, j, T, &l, &r, &s)) { status[lo + j] |= MBLS_VBG_BAD_MSG; continue; }
        if (l != j) continue;
        head[lo + G] = (uint32_t)(lo + start); entry[lo + G] = msg_idx[lo + j];
        for (uint32_t t = 0; t < s; t++) { rlo[lo + start + t] = (uint32_t)(lo + start); rhi[lo + start + t] = (uint32_t)(lo + start + s); }
        start += s; G++;
    }
    for (uint32_t j = 0; j < (uint32_t)m; j++) {
        uint32_t l, r, s;
        if (!vbg_lane_walk(msg_idx + lo, (uint32_t)m, j, T, &l, &r, &s)) continue;
        uint32_t g = 0;
        while (entry[lo + g] != msg_idx[lo + j]) g++;
        pos[lo + j] = head[lo + g] + r;
    }
    return G;
}
// is batch b SOUND: its range is sound and it owns every set of it alone under the map (ragged layouts; a uniform layout has no map and cannot overlap). Unsound
// batches join nothing -- they are rejected by the batch entries' own rules (mbls_vmb.h) -- and sets without an owner join nothing.
MBLS_VFN bool vbg_batch_sound(const uint32_t* map, const uint32_t* off, uint32_t k, uint64_t n, uint64_t b, uint64_t* lo, uint64_t* hi) {
    if (!vmb_range(off, k, n, b, lo, hi)) return false;
    if (!off) return true;
    for (uint64_t j = *lo; j < *hi; j++) if (map[j] != (uint32_t)b) return false;
    return true;
}

// ---- the Miller items of the grouped route: [0, B) the batches' (S_b, -G1) pairs, [B, B + bound) the groups -- global group r = goff[b] + g, goff[0 .. B] the
// exclusive scan of the batches' group counts, D = goff[B] the live groups, which stays on the device
// the batch global group r belongs to: the b with goff[b] <= r < goff[b + 1] (binary search; empty batches repeat an offset and are stepped over). false: r >= D.
MBLS_VFN bool vbg_group_batch_of(const uint32_t* goff, uint64_t B, uint64_t r, uint64_t* b) {
    if (!B || r >= (uint64_t)goff[B]) return false;
    uint64_t lo = 0, hi = B;                  // invariant: goff[lo] <= r < goff[hi]
    while (hi - lo > 1) { const uint64_t mid = lo + (hi - lo) / 2; if ((uint64_t)goff[mid] <= r) lo = mid; else hi = mid; }
    *b = lo; return true;
}
// fail closed: a batch whose groups reach beyond the group items the call was sized with (the caller's max_groups was too small) is rejected with
// MBLS_ST_BAD_MSG_RANGE -- its groups at or above `bound` have no Miller item --; its neighbours in front keep theirs
MBLS_VFN bool vbg_overflow(const uint32_t* goff, uint64_t b, uint64_t bound) { return (uint64_t)goff[b + 1] > bound; }
// is global group r a LIVE Miller item: it exists, it has an item, and its batch did not overflow
MBLS_VFN bool vbg_group_live(const uint32_t* goff, uint64_t B, uint64_t bound, uint64_t r, uint64_t* b) {
    if (r >= bound || !vbg_group_batch_of(goff, B, r, b)) return false;
    return !vbg_overflow(goff, *b, bound);
}

// ---- routing and sizes
// the longest batch the host has to reckon with: sets_per_batch, what a host entry has counted, or (a device-side table) all n sets
MBLS_VFN uint64_t vbg_longest(uint64_t n, uint32_t spb, uint64_t longest_known) { return longest_known ? longest_known : spb ? (uint64_t)spb : n; }
// What the host knows about the number of distinct (batch, entry) pairs of a call: at most one per set; at most T per batch WHERE no batch can be larger than the
// cap (a larger batch is not grouped and has one group per valid set, which may be more than T); at most sets_per_batch per batch where the layout is uniform
// (spb != 0); and the caller's promise where it makes one (max_groups != 0). Host entries pass their exact count as max_groups.
MBLS_VFN uint64_t vbg_bound(uint64_t n, uint64_t B, uint64_t T, uint32_t spb, uint64_t max_groups, uint64_t longest) {
    uint64_t v = n;
    if (vbg_batch_grouped(longest) && B * T < v) v = B * T;       // (B, T < 2^32)
    if (spb && B * (uint64_t)spb < v) v = B * (uint64_t)spb;
    if (max_groups && max_groups < v) v = max_groups;
    return v;
}
// mbls_ctx_set_vm_grouping: 1 grouped, 2 per set, 0 auto -- the rule of the shared-message entries (mbls_vms.h vms_grouped) on the bound: a count, not a measurement
MBLS_VFN bool vbg_grouped(uint64_t n, uint64_t bound, int mode) { return mode == 1 ? true : mode == 2 ? false : 2 * bound <= n; }
// tree levels of the grouped route's key sums: a group holds at most a batch's sets, and only batches of at most the cap are grouped (larger ones have groups of one)
MBLS_VFN uint32_t vbg_key_levels(uint64_t longest) { return vmb_levels(longest < (uint64_t)MBLS_VBG_MAX_SETS ? longest : (uint64_t)MBLS_VBG_MAX_SETS); }
// tree levels of the per-batch products over the group items: a batch has at most `longest` groups and at most `bound`
MBLS_VFN uint32_t vbg_product_levels(uint64_t longest, uint64_t bound) { return vmb_levels(longest < bound ? longest : bound); }
MBLS_VFN uint64_t vbg_miller_items(uint64_t n, uint64_t B, uint64_t bound, bool grouped) { return grouped ? B + bound : n + B; }
// Workspace of the grouped route: the sets [0, n) -- over which the Miller items [0, B + bound) are laid once the keys have moved --, the positions
// [pbase, pbase + n), the tail's 2 B items (signature pair values, then the batches' products) behind them, and for _locate two shadow items per set behind those.
MBLS_VFN uint64_t vbg_position_base(uint64_t n, uint64_t B, uint64_t bound) { return n > B + bound ? n : B + bound; }
MBLS_VFN uint64_t vbg_tail_first(uint64_t n, uint64_t B, uint64_t bound) { return vbg_position_base(n, B, bound) + n; }
MBLS_VFN uint64_t vbg_shadow_first(uint64_t n, uint64_t B, uint64_t bound) { return vbg_tail_first(n, B, bound) + 2 * B; }
MBLS_VFN uint64_t vbg_workspace_items(uint64_t n, uint64_t B, uint64_t bound, bool grouped, bool locate) {
    if (!grouped) return vmb_workspace_items(n, B, false) + (locate ? n : 0);      // (mbls_vml.h vml_workspace_items: the message phase is a gather, no lane pairs)
    return vbg_shadow_first(n, B, bound) + (locate ? 2 * n : 0);
}
// The span form (mbls_verify_multiple_batches_committee_span_msgtable*) under a split key sum (mbls_vcs.h, THE SPLIT): the 2 P n partial sums stand behind
// everything the call lays out above -- per-set route: sets, signature pairs, the batches' view, the locate shadows; grouped route: group items, positions, tail,
// two shadows per set --, lane g of k_vcs_partial_d at item vbg_partial_first + g, and its status word at the same index of the context's status words (behind
// the sets' and batches' words and the candidate flags, which end at 2 n + 2 B <= this item). The call then takes vbg_partial_first + vcs_extra_items(n, P) items.
MBLS_VFN uint64_t vbg_partial_first(uint64_t n, uint64_t B, uint64_t bound, bool grouped, bool locate) { return vbg_workspace_items(n, B, bound, grouped, locate); }
// the words of the group arrays a call needs per array (pos, rlo, rhi, head, entry over the sets; gcount and goff over the batches share the sixth)
MBLS_VFN uint64_t vbg_group_words(uint64_t n, uint64_t B) { const uint64_t a = n, b = 2 * B + 2; return a > b ? a : b; }
#endif

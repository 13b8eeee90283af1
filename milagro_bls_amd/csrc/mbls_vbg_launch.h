// mbls_vbg_launch.h -- the kernels of the grouped route of mbls_verify_multiple_batches_committee_msgtable* as the host path sees them (include/mbls.h; the rules:
// mbls_vbg.h). They are compiled in a translation unit of their own (mbls_vbg.hip), hence into a code object of their own, as mbls_cms.hip and mbls_vcs.hip are:
// the code object of mbls_kernels.hip is byte for byte what it is without these entries. vbg_impl enqueues them through these functions.
#ifndef MBLS_VBG_LAUNCH_H
#define MBLS_VBG_LAUNCH_H
#include <hip/hip_runtime.h>
#include "mbls_ops.h"
#include "mbls_vbg.h"

// the group arrays of a call, each over the sets [0, n) except gcount [0, B) and goff [0, B]
struct mbls_vbg_arrays { uint32_t* pos; uint32_t* rlo; uint32_t* rhi; uint32_t* head; uint32_t* entry; uint32_t* gcount; uint32_t* goff; };

// one wave per batch: positions, ranges, batch-local group records and the group count of every sound batch; MBLS_ST_BAD_MSG_RANGE for owned sets that name nothing.
// The arrays over the sets must read MBLS_VBG_NONE and gcount 0 beforehand (the launcher does not clear them).
void mbls_vbg_launch_group(const uint32_t* msg_idx, uint64_t T, const uint32_t* off, uint32_t spb, uint64_t B, uint64_t n, const uint32_t* map, mbls_vbg_arrays a,
                           uint32_t* status, hipStream_t s);
// one lane per set: the blinded key (slot APK of item i) -> position item pbase + pos[i]
void mbls_vbg_launch_scatter(mbls_ws ws, const uint32_t* pos, uint64_t n, uint64_t pbase, hipStream_t s);
// `levels` levels of the per-group key sums over the positions (wp = the workspace seen from the first position)
void mbls_vbg_launch_key_trees(mbls_ws wp, const uint32_t* rlo, const uint32_t* rhi, uint64_t n, uint32_t levels, hipStream_t s);
// the group items [B, B + bound): H from the table, the key from the head of the group's range, the item -> batch map; idle items get infinity and 1 in slot F; *live <- the items that have a pair
void mbls_vbg_launch_heads(mbls_ws ws, const uint32_t* tab, uint64_t tstride, const uint32_t* flags, uint64_t T, mbls_vbg_arrays a, const uint32_t* off, uint32_t spb,
                           uint64_t B, uint64_t n, uint64_t bound, uint64_t pbase, uint32_t* imap, uint32_t* st_batch, uint32_t* live, hipStream_t s);
// one lane per batch: signature pair value -> tail item b, the product of its group items (1 without any) -> tail item B + b, table faults and overflow -> status
void mbls_vbg_launch_gather(mbls_ws ws, mbls_vbg_arrays a, const uint32_t* off, uint32_t spb, uint64_t B, uint64_t n, uint64_t bound, uint64_t tail,
                            uint32_t* st_batch, const uint32_t* owned, hipStream_t s);
// _locate, one lane per set (wsa = the workspace seen from the first shadow item): the answers that need no pairing, the candidate flags, a candidate's H
void mbls_vbg_launch_mark(mbls_ws wsa, const uint32_t* tab, uint64_t tstride, const uint32_t* flags, const uint32_t* msg_idx, uint64_t T, const uint32_t* map,
                          const uint32_t* off, uint32_t spb, uint64_t B, uint64_t n, const uint32_t* st_set, const uint32_t* owned, const uint8_t* batch_results,
                          uint32_t* cand, uint8_t* set_results, uint32_t* set_status, hipStream_t s);
#endif

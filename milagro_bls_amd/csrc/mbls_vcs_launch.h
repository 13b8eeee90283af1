// mbls_vcs_launch.h -- the kernels of verify_multiple over committee spans as the host path sees them (include/mbls.h, mbls_verify_multiple_committee_span_msgtable*;
// the rules: mbls_vcs.h). They are compiled in a translation unit of their own (mbls_vcs.hip), hence into a code object of their own: the code objects of
// mbls_kernels.hip and mbls_cms.hip are byte for byte what they are without these entries. verify_multiple_impl enqueues them through these functions.
#ifndef MBLS_VCS_LAUNCH_H
#define MBLS_VCS_LAUNCH_H
#include <hip/hip_runtime.h>
#include "mbls_ops.h"
#include "mbls_vcs.h"

// one wave per set: a single-key set's one index, otherwise wave_cms_expand unchanged -> the set's direct list, missing list and record
void mbls_vcs_launch_expand(const uint32_t* crecs, uint64_t ccount, const uint32_t* members, const uint32_t* cmt_ids, uint64_t n_cmt_ids, const uint32_t* cmt_off,
                            const uint8_t* bits, uint32_t bits_stride, int mode, uint32_t* list, uint64_t stride, uint32_t* item_recs, uint64_t n, hipStream_t s);
// P = 1: one lane per set, lane_aggregate_cms with the status word cut by vmc_key_status
void mbls_vcs_launch_aggregate(mbls_ws ws, const uint32_t* recs, uint64_t tsize, const uint32_t* list, uint64_t stride, const uint32_t* item_recs, const uint32_t* crecs,
                               const uint32_t* cmt_ids, const uint32_t* cmt_off, uint32_t* park, uint64_t park_stride, uint32_t* status, uint64_t n, hipStream_t s);
// P > 1: one lane per (set, list, chunk) sums its chunk into workspace item `base` + lane and leaves its status word in st_sub[lane]; then one lane per set adds the
// partial sums and the masked segments' cached sums into the set's own APK slots and ORs the direct chunks' status bits into status
void mbls_vcs_launch_split(mbls_ws ws, uint64_t base, uint32_t P, const uint32_t* recs, uint64_t tsize, const uint32_t* list, uint64_t stride, const uint32_t* item_recs,
                           const uint32_t* crecs, const uint32_t* cmt_ids, const uint32_t* cmt_off, uint32_t* st_sub, uint32_t* status, uint64_t n, hipStream_t s);
#endif

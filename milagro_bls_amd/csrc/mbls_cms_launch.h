// mbls_cms_launch.h -- the two kernels of the committee-span entries as the host path sees them. k_cms_expand and k_aggregate_cms_d are compiled in a translation
// unit of their own (mbls_cms.hip), hence into a code object of their own: the code object of mbls_kernels.hip, which holds every kernel of the other entries, is
// byte for byte the one it is without the span entries. The pass in mbls_kernels.hip enqueues them through these two functions.
#ifndef MBLS_CMS_LAUNCH_H
#define MBLS_CMS_LAUNCH_H
#include <hip/hip_runtime.h>
#include "mbls_ops.h"
#include "mbls_cms.h"

// one wave per item: (committee ids, concatenated bitfield) -> the item's direct list, missing list and record (mbls_cms_lanes.h wave_cms_expand)
void mbls_cms_launch_expand(const uint32_t* crecs, uint64_t ccount, const uint32_t* members, const uint32_t* cmt_ids, uint64_t n_cmt_ids, const uint32_t* cmt_off,
                            const uint8_t* bits, uint32_t bits_stride, int mode, uint32_t* list, uint64_t stride, uint32_t* item_recs, uint64_t n, hipStream_t s);
// one lane per item: the key sum from both lists, the cached sums and the parked point; the status bits are ORed into status (mbls_cms_lanes.h lane_aggregate_cms)
void mbls_cms_launch_aggregate(mbls_ws ws, const uint32_t* recs, uint64_t tsize, const uint32_t* list, uint64_t stride, const uint32_t* item_recs, const uint32_t* crecs,
                               const uint32_t* cmt_ids, const uint32_t* cmt_off, uint32_t* park, uint64_t park_stride, uint32_t* status, uint64_t n, hipStream_t s);
#endif

// mbls_cms.hip -- the kernels of the committee-span entries (include/mbls.h "committee spans"; arithmetic: mbls_cms.h, device bodies: mbls_cms_lanes.h) and the two
// functions that enqueue them (mbls_cms_launch.h). A translation unit of its own: its code object carries its own copies of the generated routines the key sum
// calls, and the code object of mbls_kernels.hip stays what it is without these entries.
//   k_cms_expand       one wave per item walks the item's segments, decides each segment's route and leaves the direct list, the missing list and the record
//   k_aggregate_cms_d  one lane per item sums both lists with the generated indexed key sum, adds the masked committees' cached sums and forms the status word
//                      from the final point
#include <hip/hip_runtime.h>
#include "mbls_cms_launch.h"
#include "mbls_cms_lanes.h"

#if defined(MBLS_NO_ASM) || defined(MBLS_NO_FP2_ASM) || defined(MBLS_NO_LDS_STATE)
#error "libmbls_hip.so cannot be built with MBLS_NO_ASM / MBLS_NO_FP2_ASM / MBLS_NO_LDS_STATE: the host side depends on the generated routines"
#endif
#if defined(__HIP_DEVICE_COMPILE__) && !MBLS_DEVICE_ASM
#error "device pass without the generated routines"
#endif

#define CMS_WG 64
// one wave per SIMD, like the key-sum kernels of mbls_kernels.hip: the generated routine owns 512 registers per lane
#define CMS_LB __launch_bounds__(CMS_WG, 1)

__global__ void __launch_bounds__(CMS_WG) k_cms_expand(const uint32_t* crecs, uint64_t ccount, const uint32_t* members, const uint32_t* cmt_ids, uint64_t n_cmt_ids,
                                                       const uint32_t* cmt_off, const uint8_t* bits, uint32_t bits_stride, int mode, uint32_t* list, uint64_t stride,
                                                       uint32_t* item_recs, uint64_t n) {
    const uint64_t i = blockIdx.x; if (i >= n) return;
    wave_cms_expand(i, threadIdx.x, crecs, ccount, members, cmt_ids, n_cmt_ids, cmt_off, bits, bits_stride, mode, list, stride, item_recs);
}
__global__ void CMS_LB k_aggregate_cms_d(mbls_ws ws, const uint32_t* recs, uint64_t tsize, const uint32_t* list, uint64_t stride, const uint32_t* item_recs,
                                         const uint32_t* crecs, const uint32_t* cmt_ids, const uint32_t* cmt_off, uint32_t* park, uint64_t park_stride,
                                         uint32_t* status, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * CMS_WG + threadIdx.x; if (i >= n) return;
#if MBLS_DEVICE_ASM            // (the host pass does not see the body)
    uint32_t st = lane_aggregate_cms(ws, i, threadIdx.x, recs, tsize, list, stride, item_recs, crecs, cmt_ids, cmt_off, park, park_stride);
    if (st) atomicOr(status + i, st);
#endif
}

void mbls_cms_launch_expand(const uint32_t* crecs, uint64_t ccount, const uint32_t* members, const uint32_t* cmt_ids, uint64_t n_cmt_ids, const uint32_t* cmt_off,
                            const uint8_t* bits, uint32_t bits_stride, int mode, uint32_t* list, uint64_t stride, uint32_t* item_recs, uint64_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_cms_expand, dim3((unsigned)n), dim3(CMS_WG), 0, s, crecs, ccount, members, cmt_ids, n_cmt_ids, cmt_off, bits, bits_stride, mode, list, stride,
                       item_recs, n);
}
void mbls_cms_launch_aggregate(mbls_ws ws, const uint32_t* recs, uint64_t tsize, const uint32_t* list, uint64_t stride, const uint32_t* item_recs, const uint32_t* crecs,
                               const uint32_t* cmt_ids, const uint32_t* cmt_off, uint32_t* park, uint64_t park_stride, uint32_t* status, uint64_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_aggregate_cms_d, dim3((unsigned)((n + CMS_WG - 1) / CMS_WG)), dim3(CMS_WG), 0, s, ws, recs, tsize, list, stride, item_recs, crecs, cmt_ids, cmt_off,
                       park, park_stride, status, n);
}

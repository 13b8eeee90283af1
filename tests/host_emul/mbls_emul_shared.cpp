// mbls_emul_shared.cpp -- TEST INFRASTRUCTURE, beside mbls_emul.cpp: the shared-message pipeline (include/mbls.h, mbls_*_shared_msgs) on the lane bodies of the HIP
// kernels, compiled as plain C++ and run one "lane" at a time on the CPU: hash the LIST (in pieces, in workspace items [0, piece) like the GPU), export the points
// to a table (lane_h_export), gather per item (lane_h_gather), then the rest of the pipeline. Not a fallback: the product library never loads this file.
#define MBLS_HOST_EMUL 1
#include <stdlib.h>
#include <string.h>
#include "../../milagro_bls_amd/csrc/mbls_ops.h"

extern "C" {
// msgs: the list (mlen bytes each, or msgs[moff[j] .. moff[j+1]) with n_msgs + 1 offsets); item i's message is message msg_idx[i]. piece_items: messages per
// piece of the list hash (0: all at once). The rules of the device entries: an index >= n_msgs, or a message whose range runs backwards or is 2^32 bytes or more,
// rejects the items concerned with MBLS_ST_BAD_MSG_RANGE and gives them H of the empty message.
void emul_verify_batch_shared(const uint8_t* sigs, const uint8_t* msgs, uint32_t mlen, const uint64_t* moff, uint64_t n_msgs, const uint32_t* msg_idx,
                              const uint8_t* pks, int fmt, const uint32_t* offsets, uint64_t n, uint32_t k, int mode, uint64_t piece_items,
                              uint8_t* results, uint32_t* status) {
    const uint64_t piece = piece_items && piece_items < n_msgs ? piece_items : (n_msgs ? n_msgs : 1);
    mbls_ws ws; ws.stride = n > piece ? n : piece; ws.w = (uint32_t*)calloc((size_t)MBLS_SLOT_COUNT * 12 * ws.stride, 4);
    const uint64_t tstride = n_msgs + 1;
    uint32_t* tab = (uint32_t*)calloc((size_t)MBLS_H_DWORDS * tstride, 4);
    uint32_t* flags = (uint32_t*)calloc(tstride, 4);
    uint32_t* st_list = (uint32_t*)calloc(tstride, 4);
    const uint32_t pkb = fmt == MBLS_PK_COMPRESSED ? 48 : 96;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t first = offsets ? offsets[i] : (uint64_t)k * i; uint32_t cnt = offsets ? offsets[i + 1] - offsets[i] : k;
        lane_aggregate(ws, i, pks + pkb * first, cnt, fmt, mode, &status[i]);
    }
    for (uint64_t i = 0; i < n; i++) lane_sig(ws, i, sigs + 96 * i, &status[i]);
    // the list: entry 0 = the empty message, then piece after piece in workspace items [0, piece) (slot H only: the key sums and signatures above stay)
    lane_hash(ws, 0, msgs, 0);
    lane_h_export(ws, 0, tab, tstride, 0, flags, st_list);
    for (uint64_t first = 0; first < n_msgs; first += piece) {
        const uint64_t m = n_msgs - first < piece ? n_msgs - first : piece;
        for (uint64_t j = 0; j < m; j++) {
            const uint8_t* p = msgs + (uint64_t)mlen * (first + j); uint32_t len = mlen;
            st_list[1 + first + j] = 0;
            if (moff) {
                const uint64_t a = moff[first + j], b = moff[first + j + 1];
                const bool bad = b < a || b - a > 0xFFFFFFFFull;
                p = msgs + (bad ? 0 : a); len = bad ? 0u : (uint32_t)(b - a);
                if (bad) st_list[1 + first + j] = MBLS_ST_BAD_MSG_RANGE;
            }
            lane_hash(ws, j, p, len);
        }
        for (uint64_t j = 0; j < m; j++) lane_h_export(ws, j, tab, tstride, 1 + first + j, flags, st_list + 1 + first);
    }
    for (uint64_t i = 0; i < n; i++) status[i] |= lane_h_gather(ws, i, tab, tstride, flags, msg_idx[i], n_msgs);
    for (uint64_t i = 0; i < n; i++) lane_miller(ws, i);
    for (uint64_t i = 0; i < n; i++) lane_final(ws, i, &status[i], &results[i]);
    free(ws.w); free(tab); free(flags); free(st_list);
}
}

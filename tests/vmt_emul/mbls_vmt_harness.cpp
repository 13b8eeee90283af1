// Host harness of milagro_bls_amd/csrc/mbls_vmt.h (tests/test_vm_msgtable_cpu.py): from the sets' table indices to the Miller items of a verify_multiple call
// over a resident message table -- count, exclusive scan, scatter (mbls_vms.h, with the table's size T as the list length), then flag, the scan of the flags,
// named and heads exactly as k_vmt_flag / k_vms_scan / k_vmt_named / k_vmt_heads run them.
// stdin, one case per line:  n T miller_items idx_0 .. idx_{n-1}
// stdout, per case:          D overflow idle_from | named_0 .. named_{D-1} | live_r idx_r pos_r map_r   for r < miller_items
//   overflow: vmt_overflow(D, miller_items); idle_from: the first item index r for which vmt_wave_idle(r, D) holds (miller_items: none);
//   live_r / idx_r / pos_r: what vmt_head gives Miller item r; map_r: the group the scatter's map names at position pos_r (live items: must be idx_r)
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../milagro_bls_amd/csrc/mbls_vmt.h"

// k_vms_scan: the lanes' chunks, the scan of the chunk sums, the chunks written (out[0 .. M])
static void scan(const std::vector<uint32_t>& in, uint64_t M, std::vector<uint32_t>& out) {
    const uint32_t L = MBLS_VMS_SCAN_LANES;
    std::vector<uint32_t> part(L), sum(L);
    for (uint32_t t = 0; t < L; t++) { uint64_t lo, hi; vms_scan_chunk(M, L, t, &lo, &hi); uint32_t s = 0; for (uint64_t j = lo; j < hi; j++) s += in[j]; part[t] = sum[t] = s; }
    for (uint32_t d = 1; d < L; d *= 2) { std::vector<uint32_t> nx(part); for (uint32_t t = d; t < L; t++) nx[t] = part[t] + part[t - d]; part.swap(nx); }
    for (uint32_t t = 0; t < L; t++) {
        uint64_t lo, hi; vms_scan_chunk(M, L, t, &lo, &hi);
        uint32_t run = part[t] - sum[t];
        for (uint64_t j = lo; j < hi; j++) { out[j] = run; run += in[j]; }
        if (t == L - 1) out[M] = part[t];
    }
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        uint64_t n, T, items;
        in >> n >> T >> items;
        std::vector<uint32_t> idx(n);
        for (auto& x : idx) { uint64_t v; in >> v; x = (uint32_t)v; }
        const uint64_t W = vmt_group_words(T);
        std::vector<uint32_t> cnt(W, 0), cur(W, 0), off(W, 0), flag(W, 0), roff(W, 0), named(T ? T : 1, 0xDEADBEEFu);
        // k_vms_count, k_vms_scan, k_vms_scatter (the map alone: the sums are tests/vms_emul's subject)
        for (uint64_t i = 0; i < n; i++) { const uint32_t g = vms_group(idx[i], T); if (g != MBLS_VMS_NO_GROUP) cnt[g]++; }
        scan(cnt, T, off);
        std::vector<uint32_t> map(n ? n : 1, MBLS_VMS_NO_GROUP);
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t g = vms_group(idx[i], T);
            if (g == MBLS_VMS_NO_GROUP) continue;
            const uint64_t p = vms_position(off.data(), g, cur[g]++);
            if (p < n) map[p] = g;
        }
        // k_vmt_flag, k_vms_scan over the flags, k_vmt_named
        for (uint64_t j = 0; j < T; j++) flag[j] = vmt_flag(cnt[j]);
        scan(flag, T, roff);
        for (uint64_t j = 0; j < T; j++) { uint32_t slot; if (vmt_named_slot(flag.data(), roff.data(), j, &slot) && (uint64_t)slot < T) named[slot] = (uint32_t)j; }
        const uint64_t D = roff[T];
        uint64_t idle_from = items;
        for (uint64_t r = 0; r < items; r++) if (vmt_wave_idle(r, (uint32_t)D)) { idle_from = r; break; }
        printf("%llu %d %llu |", (unsigned long long)D, vmt_overflow(D, items) ? 1 : 0, (unsigned long long)idle_from);
        for (uint64_t r = 0; r < D; r++) printf(" %u", named[r]);
        printf(" |");
        // k_vmt_heads
        for (uint64_t r = 0; r < items; r++) {
            uint32_t e; uint64_t pos;
            const bool live = vmt_head(named.data(), off.data(), D, r, &e, &pos);
            printf(" %d %u %llu %u", live ? 1 : 0, e, (unsigned long long)pos, live && pos < n ? map[pos] : MBLS_VMS_NO_GROUP);
        }
        printf("\n");
    }
    return 0;
}

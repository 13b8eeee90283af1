// Host harness of milagro_bls_amd/csrc/mbls_vms.h (tests/test_vm_shared_cpu.py): the grouping of the shared-message verify_multiple -- count, exclusive scan,
// scatter, per-message tree levels, heads -- exactly as the kernels k_vms_count / k_vms_scan / k_vms_scatter / k_g1_seg_tree_d / k_vms_heads run it, over 64-bit
// integers with `+` as the group operation. The order in which the sets of a group take their tickets is the caller's (the GPU's is whatever the atomics make it).
// stdin, one case per line:  n n_msgs order_seed idx_0 .. idx_{n-1}        (order_seed 0: sets in index order; else a seeded permutation)
// stdout, per case:          head_0 some_0 .. head_{M-1} some_{M-1} | levels bad_sets placed double_or_missing out_of_range
//   head_g / some_g: what Miller item g would get (the sum at the head of g's range; some = 0: no set names g -- infinity);
//   bad_sets: sets that joined no group; placed: positions written; double_or_missing: positions of a range written twice or never, and sets placed outside
//   their message's range; out_of_range: tree steps that read outside the owner's range
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../milagro_bls_amd/csrc/mbls_vms.h"

static uint64_t val(uint64_t j) {      // set j's start value (tests/test_vm_shared_cpu.py computes the same)
    uint64_t z = (j + 1) * 0x9E3779B97F4A7C15ull;
    z ^= z >> 29; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 32;
    return z;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        uint64_t n, M, seed;
        in >> n >> M >> seed;
        std::vector<uint32_t> idx(n);
        for (auto& x : idx) { uint64_t v; in >> v; x = (uint32_t)v; }
        // k_vms_count
        std::vector<uint32_t> cnt(M + 1, 0), cur(M + 1, 0), off(M + 1, 0);
        uint64_t bad = 0;
        for (uint64_t i = 0; i < n; i++) { const uint32_t g = vms_group(idx[i], M); if (g == MBLS_VMS_NO_GROUP) bad++; else cnt[g]++; }
        // k_vms_scan: the lanes' chunks, the scan of the chunk sums, the chunks written
        {
            const uint32_t T = MBLS_VMS_SCAN_LANES;
            std::vector<uint32_t> part(T), sum(T);
            for (uint32_t t = 0; t < T; t++) { uint64_t lo, hi; vms_scan_chunk(M, T, t, &lo, &hi); uint32_t s = 0; for (uint64_t j = lo; j < hi; j++) s += cnt[j]; part[t] = sum[t] = s; }
            for (uint32_t d = 1; d < T; d *= 2) { std::vector<uint32_t> nx(part); for (uint32_t t = d; t < T; t++) nx[t] = part[t] + part[t - d]; part.swap(nx); }
            for (uint32_t t = 0; t < T; t++) {
                uint64_t lo, hi; vms_scan_chunk(M, T, t, &lo, &hi);
                uint32_t run = part[t] - sum[t];
                for (uint64_t j = lo; j < hi; j++) { off[j] = run; run += cnt[j]; }
                if (t == T - 1) off[M] = part[t];
            }
        }
        // k_vms_scatter, the sets arriving in the order the case names
        std::vector<uint64_t> order(n);
        for (uint64_t i = 0; i < n; i++) order[i] = i;
        if (seed) { uint64_t s = seed; for (uint64_t i = n; i > 1; i--) { s = s * 6364136223846793005ull + 1442695040888963407ull; std::swap(order[i - 1], order[(s >> 33) % i]); } }
        std::vector<uint64_t> pos(n ? n : 1, 0);
        std::vector<uint32_t> map(n ? n : 1, MBLS_VMS_NO_GROUP), written(n ? n : 1, 0);
        uint64_t placed = 0, wrong = 0;
        for (uint64_t q = 0; q < n; q++) {
            const uint64_t i = order[q];
            const uint32_t g = vms_group(idx[i], M);
            if (g == MBLS_VMS_NO_GROUP) continue;
            const uint64_t p = vms_position(off.data(), g, cur[g]++);
            if (p >= n) { wrong++; continue; }
            uint64_t lo, hi; vms_range(off.data(), g, &lo, &hi);
            if (p < lo || p >= hi) wrong++;
            map[p] = g; pos[p] = val(i); written[p]++; placed++;
        }
        for (uint64_t g = 0; g < M; g++) { uint64_t lo, hi; vms_range(off.data(), g, &lo, &hi); for (uint64_t p = lo; p < hi; p++) if (written[p] != 1) wrong++; }
        // k_g1_seg_tree_d, level after level (a level reads only what the level before left)
        const uint32_t levels = vms_levels(n, 0);
        uint64_t outside = 0, half = 1;
        for (uint32_t l = 0; l < levels; l++, half *= 2) {
            std::vector<uint64_t> nx(pos);
            for (uint64_t p = 0; p < n; p++) {
                uint64_t lo, hi;
                if (!vms_owner_range(map.data(), off.data(), M, n, p, &lo, &hi)) continue;
                if (!vmb_takes_partner(p, lo, hi, half)) continue;
                if (p + half >= hi || p + half >= n) { outside++; continue; }
                nx[p] = pos[p] + pos[p + half];
            }
            pos.swap(nx);
        }
        // k_vms_heads
        const uint64_t Mm = vms_miller_items(M);
        for (uint64_t j = 0; j < Mm; j++) {
            const bool some = j < M && cnt[j] != 0;
            printf("%llu %d ", (unsigned long long)(some ? pos[off[j]] : 0), some ? 1 : 0);
        }
        printf("| %u %llu %llu %llu %llu\n", levels, (unsigned long long)bad, (unsigned long long)placed, (unsigned long long)wrong, (unsigned long long)outside);
    }
    return 0;
}

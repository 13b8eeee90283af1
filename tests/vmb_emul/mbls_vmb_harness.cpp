// mbls_vmb_harness.cpp -- milagro_bls_amd/csrc/mbls_vmb.h (the segment arithmetic of mbls_verify_multiple_batches*) built with the host compiler and run over
// integers with `+` as the operation, the way the kernels of mbls_kernels.hip run it over G2 points and Fp12 values: the map (k_vmb_set_map), the tree levels
// (k_g2_seg_tree_d / k_f12_seg_tree_d), the status fold's ownership count (k_vmb_status_fold) and the gather's verdict (k_vmb_gather).
// stdin: one table per line: "B n k order off_0 ... off_B" (k > 0: uniform layout, no offsets follow; order: 0 = batches claim their sets in index order,
// 1 = in reverse -- claims race on the device). stdout, per table: one line "head rejected crossed" triples, one per batch:
//   head     = the value at the head of the batch's range after the levels (0 for an empty or faulty range), values start as val(j) (see below)
//   rejected = the gather's verdict
//   crossed  = 1 when a step that wrote to a set of this batch read a set that is not this batch's by the map, or outside its range
// With the argument "v": the host entries' table check (see main).
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../../milagro_bls_amd/csrc/mbls_vmb.h"

static uint64_t val(uint64_t j) { uint64_t z = (j + 1) * 0x9E3779B97F4A7C15ull; z ^= z >> 29; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 32; return z; }

int main(int argc, char** argv) {
    unsigned long long B, n, k, order;
    if (argc > 1 && argv[1][0] == 'v') {          // "v": vmb_offsets_ok, what the host entries run; stdin "B n off_0 ... off_B" per line -> "ok longest"
        while (scanf("%llu %llu", &B, &n) == 2) {
            std::vector<uint32_t> off(B + 1);
            for (auto& o : off) { unsigned long long v; if (scanf("%llu", &v) != 1) return 2; o = (uint32_t)v; }
            uint64_t longest = 0;
            const bool ok = vmb_offsets_ok(off.data(), B, n, &longest);
            printf("%d %llu\n", ok ? 1 : 0, (unsigned long long)(ok ? longest : 0));
        }
        return 0;
    }
    while (scanf("%llu %llu %llu %llu", &B, &n, &k, &order) == 4) {
        std::vector<uint32_t> off;
        if (!k) { off.resize(B + 1); for (auto& o : off) { unsigned long long v; if (scanf("%llu", &v) != 1) return 2; o = (uint32_t)v; } }
        const uint32_t* po = k ? nullptr : off.data();
        std::vector<uint32_t> map(n ? n : 1, MBLS_VMB_NO_OWNER), owned(B ? B : 1, 0), crossed(B ? B : 1, 0);
        if (po)
            for (uint64_t t = 0; t < B; t++) {
                const uint64_t b = order ? B - 1 - t : t;
                uint64_t lo, hi;
                if (!vmb_range(po, 0, n, b, &lo, &hi)) continue;
                for (uint64_t j = lo; j < hi; j++) map[j] = vmb_claim(map[j], (uint32_t)b);
            }
        const uint32_t* pm = po ? map.data() : nullptr;
        std::vector<uint64_t> v(n ? n : 1);
        for (uint64_t j = 0; j < n; j++) v[j] = val(j);
        const uint64_t longest = po ? n : k;
        for (uint64_t half = 1; half < longest; half *= 2) {
            // a level is one launch: every lane reads the state the previous level left (a lane's partner is never a writer of the same level and owner)
            std::vector<uint64_t> nv(v);
            for (uint64_t j = 0; j < n; j++) {
                uint64_t lo, hi;
                if (!vmb_owner_range(pm, po, (uint32_t)k, B, n, j, &lo, &hi)) continue;
                if (!vmb_takes_partner(j, lo, hi, half)) continue;
                const uint64_t p = j + half, b = po ? map[j] : j / k;
                if (p >= n || p < lo || p >= hi || (po && map[p] != map[j])) crossed[b] = 1;
                if (p < n) nv[j] = v[j] + v[p];
            }
            v.swap(nv);
        }
        for (uint64_t j = 0; j < n; j++) {          // k_vmb_status_fold's count
            uint64_t lo, hi;
            if (po && vmb_owner_range(pm, po, (uint32_t)k, B, n, j, &lo, &hi)) owned[map[j]]++;
        }
        for (uint64_t b = 0; b < B; b++) {          // k_vmb_gather
            uint64_t lo, hi;
            int rej = 0;
            if (!vmb_range(po, (uint32_t)k, n, b, &lo, &hi)) rej = 1;
            if (!vmb_owns_all(po ? owned.data() : nullptr, b, lo, hi)) rej = 1;
            printf("%llu %d %u ", (unsigned long long)(hi > lo ? v[lo] : 0), rej, crossed[b]);
        }
        printf("| %u\n", vmb_levels(longest));
    }
    return 0;
}

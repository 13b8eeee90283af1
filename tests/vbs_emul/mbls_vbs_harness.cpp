// Host harness for the workspace layout of mbls_verify_multiple_batches_committee_span_msgtable* (include/mbls.h): a stand-alone program over the pure layout
// headers alone (mbls_vbg.h, mbls_vml.h, mbls_vcs.h), built with the host compiler under AddressSanitizer and UBSan by tests/test_vm_batches_committee_span_cpu.py.
// It sweeps (n, B, bound, P, locate, route) and, for every point, paints the item ranges and the status-word ranges the batches layout functions return into two
// arrays of exactly the plan's size, then paints the partial sums' range (vbg_partial_first, 2 P n items and as many words): a cell painted twice is an overlap, a
// write past the array is the sanitizer's. WHAT THIS DOES NOT SHOW: the regions are restated here by hand from the layout functions as vbg_impl (mbls_kernels.hip)
// uses them today -- the grouped front as max(n, B + bound), for instance --, so a region vbg_impl gains later goes unseen until it is added here; and the end of the
// partial range is not compared with a plan computed here (vbg_partial_first IS vbg_workspace_items: the comparison could not fail) -- the test holds the `end`
// this program prints to the LIBRARY's mbls_plan_verify_multiple_batches_committee_span figure instead.
// stdin: lines "n B bound P locate grouped"; stdout per line: "first end plan overlaps_items overlaps_words holes" ; no arguments: the built-in sweep, "ok <points>".
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include "../../milagro_bls_amd/csrc/mbls_vmb.h"
#include "../../milagro_bls_amd/csrc/mbls_vml.h"
#include "../../milagro_bls_amd/csrc/mbls_vbg.h"
#include "../../milagro_bls_amd/csrc/mbls_vcs.h"

struct verdict { uint64_t first, end, plan, over_items, over_words, holes; };

static void paint(std::vector<uint8_t>& a, uint64_t lo, uint64_t hi, uint64_t* over) {
    for (uint64_t i = lo; i < hi; i++) { if (a.at(i)) ++*over; a[i] = 1; }
}

// the regions of one call as vbg_impl lays them out (mbls_kernels.hip), from the layout functions alone
static verdict check(uint64_t n, uint64_t B, uint64_t bound, uint32_t P, bool locate, bool grouped) {
    verdict v = {};
    v.first = vbg_partial_first(n, B, bound, grouped, locate);
    const uint64_t extra = vcs_extra_items(n, P);
    v.end = v.first + extra;
    v.plan = vbg_workspace_items(n, B, bound, grouped, locate) + extra;
    std::vector<uint8_t> items(v.plan, 0), words(v.plan, 0);
    if (grouped) {
        // the sets [0, n) and the Miller items [0, B + bound) share the front on purpose (the keys have moved to their positions before the heads are written)
        paint(items, 0, n > B + bound ? n : B + bound, &v.over_items);
        paint(items, vbg_position_base(n, B, bound), vbg_position_base(n, B, bound) + n, &v.over_items);          // positions
        paint(items, vbg_tail_first(n, B, bound), vbg_tail_first(n, B, bound) + 2 * B, &v.over_items);            // tail: pair values, products
        if (locate) paint(items, vbg_shadow_first(n, B, bound), vbg_shadow_first(n, B, bound) + 2 * n, &v.over_items);   // A(i), B(i)
    } else {
        paint(items, 0, n, &v.over_items);                                   // sets
        paint(items, n, n + B, &v.over_items);                               // signature pairs
        paint(items, n + B, n + 2 * B, &v.over_items);                       // the batches' view: staging
        if (vmb_workspace_items(n, B, false) != n + 2 * B) v.over_items++;
        if (locate) paint(items, vml_shadow_first(n, B, false), vml_shadow_first(n, B, false) + n, &v.over_items);       // one shadow per set
    }
    // the context's status words: the sets', the batches', the ownership counts, and for locate the candidate flags
    paint(words, 0, n, &v.over_words);
    paint(words, n, n + B, &v.over_words);
    paint(words, n + B, n + 2 * B, &v.over_words);
    if (locate) paint(words, vml_flags_first(n, B), vml_flags_first(n, B) + n, &v.over_words);
    // everything the batches plan lays out ends at the first partial item
    for (uint64_t i = 0; i < v.first; i++) if (!items[i]) v.holes++;
    // the partial sums: lane g of k_vcs_partial_d -> item first + g, word first + g, g < 2 P n
    if (P > 1u) {
        const uint64_t lanes = vcs_lane_of(n - 1, 1, P - 1, P) + 1;
        if (lanes != extra) v.over_items++;
        paint(items, v.first, v.first + lanes, &v.over_items);
        paint(words, v.first, v.first + lanes, &v.over_words);
    }
    return v;
}

int main(int argc, char**) {
    if (argc > 1) {
        unsigned long long n, B, bound; unsigned P; int locate, grouped;
        while (scanf("%llu %llu %llu %u %d %d", &n, &B, &bound, &P, &locate, &grouped) == 6) {
            const verdict v = check(n, B, bound, P, locate != 0, grouped != 0);
            printf("%llu %llu %llu %llu %llu %llu\n", (unsigned long long)v.first, (unsigned long long)v.end, (unsigned long long)v.plan,
                   (unsigned long long)v.over_items, (unsigned long long)v.over_words, (unsigned long long)v.holes);
        }
        return 0;
    }
    const uint64_t ns[] = {1, 2, 3, 63, 64, 65, 200, 1025, 4096, 4097};
    const uint32_t Ps[] = {1, 2, 4, 8, 16};
    uint64_t points = 0;
    for (uint64_t n : ns)
        for (uint64_t B : {(uint64_t)1, (uint64_t)2, n / 10 + 1, n, 2 * n + 3})
            for (uint64_t bound : {(uint64_t)0, (uint64_t)1, n / 2, n})
                for (uint32_t P : Ps)
                    for (int locate = 0; locate < 2; locate++)
                        for (int grouped = 0; grouped < 2; grouped++) {
                            const verdict v = check(n, B, bound, P, locate != 0, grouped != 0);
                            if (v.over_items || v.over_words || v.holes) {
                                fprintf(stderr, "n=%llu B=%llu bound=%llu P=%u locate=%d grouped=%d: first=%llu end=%llu plan=%llu overlaps %llu/%llu holes %llu\n",
                                        (unsigned long long)n, (unsigned long long)B, (unsigned long long)bound, P, locate, grouped, (unsigned long long)v.first,
                                        (unsigned long long)v.end, (unsigned long long)v.plan, (unsigned long long)v.over_items, (unsigned long long)v.over_words,
                                        (unsigned long long)v.holes);
                                return 1;
                            }
                            points++;
                        }
    printf("ok %llu\n", (unsigned long long)points);
    return 0;
}

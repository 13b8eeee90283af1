// The draw order of the verify_multiple*_rng entries on the host (milagro_bls_amd/csrc/mbls_vmr.h): tests/test_vm_draw_cpu.py calls the header's five functions
// through this library and compares them with the reference's loop written out in Python. With -DMBLS_VMR_HARNESS_MAIN it is a program of its own that walks the
// same kinds of cases over heap buffers of exactly n status words, n scalars, B reaches and B + 1 offsets -- the form the address and undefined-behaviour
// sanitizers run.
#include <stdint.h>
#include <stdlib.h>
#include <stdio.h>
#include "../../milagro_bls_amd/csrc/mbls_vmr.h"

extern "C" {
uint64_t vr_reach(const uint32_t* st, uint64_t lo, uint64_t hi) { return vmr_reach(st, lo, hi); }
void vr_range(const uint32_t* boff, uint32_t spb, uint64_t b, uint64_t* lo, uint64_t* hi) { vmr_batch_range(boff, spb, b, lo, hi); }
uint64_t vr_plan(const uint32_t* st, const uint32_t* boff, uint32_t spb, uint64_t B, uint64_t* reach) { return vmr_plan(st, boff, spb, B, reach); }
void vr_spread(const uint64_t* drawn, const uint64_t* reach, const uint32_t* boff, uint32_t spb, uint64_t B, uint64_t* rands) { vmr_spread(drawn, reach, boff, spb, B, rands); }
void vr_close(const uint32_t* st, const uint64_t* reach, const uint32_t* boff, uint32_t spb, uint64_t B, uint8_t* set_results, uint32_t* set_status) {
    vmr_close(st, reach, boff, spb, B, set_results, set_status);
}
}

#ifdef MBLS_VMR_HARNESS_MAIN
static uint32_t rnd_state = 13579u;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }
static const uint32_t BAD[] = {MBLS_ST_BAD_SIG_ENCODING, MBLS_ST_SIG_NOT_IN_G2, MBLS_ST_BAD_SIG_ENCODING | MBLS_ST_SIG_NOT_IN_G2, MBLS_ST_SIG_NOT_IN_G2 | 0x104u};
static const uint32_t OTHER[] = {0x04u, 0x80u, 0x100u, 0xFFFFFFFCu};      // bits beside the two rejecting ones: they do not stop the loop
// fill: 0 all good, 1 all bad, 2 the first set of every batch bad, 3 the last, 4 other bits only, 5 seeded
static uint32_t word(int fill, uint64_t i, uint64_t lo, uint64_t hi) {
    const uint32_t other = (rnd() & 1u) ? OTHER[rnd() & 3u] : 0u;
    switch (fill) {
    case 0: return 0u;
    case 1: return BAD[rnd() & 3u];
    case 2: return i == lo ? BAD[rnd() & 3u] : other;
    case 3: return i + 1 == hi ? BAD[rnd() & 3u] : other;
    case 4: return OTHER[rnd() & 3u];
    default: return (rnd() % 5u) == 0u ? BAD[rnd() & 3u] | other : other;
    }
}
// sizes[0 .. B): the batches; table: an offset table of B + 1 entries, or (all sizes equal) the uniform count
static int check(const uint32_t* sizes, uint64_t B, bool table, int fill) {
    uint64_t n = 0;
    for (uint64_t b = 0; b < B; b++) n += sizes[b];
    uint32_t* boff = table ? (uint32_t*)malloc(4 * (B + 1)) : nullptr;
    if (table) { boff[0] = 0; for (uint64_t b = 0; b < B; b++) boff[b + 1] = boff[b] + sizes[b]; }
    const uint32_t spb = table ? 0xDEADu : sizes[0];
    uint32_t* st = (uint32_t*)malloc(4 * n); uint64_t* reach = (uint64_t*)malloc(8 * B); uint64_t* rands = (uint64_t*)malloc(8 * n); uint64_t* want = (uint64_t*)malloc(8 * n);
    uint8_t* sres = (uint8_t*)malloc(n); uint32_t* sst = (uint32_t*)malloc(4 * n);
    int bad = 0;
    // the reference's loops, one call after the other on one generator that counts from 1000
    uint64_t next = 1000, lo = 0;
    for (uint64_t b = 0; b < B && !bad; b++) {
        const uint64_t hi = lo + sizes[b];
        for (uint64_t i = lo; i < hi; i++) st[i] = word(fill, i, lo, hi);
        uint64_t i = lo;
        for (; i < hi && !(st[i] & (MBLS_ST_BAD_SIG_ENCODING | MBLS_ST_SIG_NOT_IN_G2)); i++) want[i] = next++;
        const uint64_t r = i - lo;
        for (; i < hi; i++) want[i] = 1;
        uint64_t glo = 7, ghi = 7;
        vmr_batch_range(boff, spb, b, &glo, &ghi);
        if (glo != lo || ghi != hi || vmr_reach(st, lo, hi) != r) { printf("range or reach B=%llu b=%llu\n", (unsigned long long)B, (unsigned long long)b); bad = 1; }
        lo = hi;
    }
    const uint64_t total = bad ? 0 : vmr_plan(st, boff, spb, B, reach);
    if (!bad && total != next - 1000) { printf("total B=%llu fill=%d\n", (unsigned long long)B, fill); bad = 1; }
    uint64_t* drawn = (uint64_t*)malloc(8 * total);
    for (uint64_t j = 0; j < total; j++) drawn[j] = 1000 + j;
    if (!bad) {
        vmr_spread(drawn, reach, boff, spb, B, rands);
        for (uint64_t i = 0; i < n; i++) if (rands[i] != want[i]) { printf("rands B=%llu fill=%d i=%llu\n", (unsigned long long)B, fill, (unsigned long long)i); bad = 1; break; }
    }
    if (!bad) {
        for (uint64_t i = 0; i < n; i++) { sres[i] = 7; sst[i] = 0xDEADBEEFu; }
        vmr_close(st, reach, boff, spb, B, sres, sst);
        for (uint64_t i = 0; i < n; i++) {
            const bool closed = want[i] == 1;        // (the generator never hands out 1)
            if (sres[i] != (closed ? 0 : 7) || sst[i] != (closed ? st[i] : 0xDEADBEEFu)) { printf("close B=%llu fill=%d i=%llu\n", (unsigned long long)B, fill, (unsigned long long)i); bad = 1; break; }
        }
        for (uint64_t i = 0; i < n; i++) sres[i] = 7;
        vmr_close(st, reach, boff, spb, B, sres, nullptr);      // the words are optional
        for (uint64_t i = 0; i < n; i++) if (sres[i] != (want[i] == 1 ? 0 : 7)) { printf("close without words\n"); bad = 1; break; }
    }
    free(boff); free(st); free(reach); free(rands); free(want); free(sres); free(sst); free(drawn);
    return bad;
}
int main() {
    long checked = 0;
    for (int fill = 0; fill < 6; fill++) {
        for (uint32_t B = 1; B <= 9; B++) {
            uint32_t sizes[9];
            // uniform counts, 0 (n = 0 with B > 0) included
            for (uint32_t spb = 0; spb <= 5; spb++) {
                for (uint32_t b = 0; b < B; b++) sizes[b] = spb;
                if (check(sizes, B, false, fill) || check(sizes, B, true, fill)) return 1;
                checked += 2;
            }
            // tables: seeded sizes, then with empty batches at the front, in the middle, at the end and everywhere
            for (int shape = 0; shape < 5; shape++) {
                for (uint32_t b = 0; b < B; b++) sizes[b] = 1 + rnd() % 6u;
                if (shape == 1) sizes[0] = 0;
                if (shape == 2) sizes[B / 2] = 0;
                if (shape == 3) sizes[B - 1] = 0;
                if (shape == 4) for (uint32_t b = 0; b < B; b += 2) sizes[b] = 0;
                if (check(sizes, B, true, fill)) return 1;
                checked++;
            }
        }
    }
    printf("ok %ld\n", checked);
    return 0;
}
#endif

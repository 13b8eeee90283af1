// The committee table's arithmetic on the host (milagro_bls_amd/csrc/mbls_cmt.h) and the committee kind of the batch description (mbls_batch.h):
// tests/test_committee_cpu.py loads this file as a shared library and compares the route, the listed positions and the slices with a Python model. Built with
// -DMBLS_CMT_HARNESS_MAIN it is a program of its own that walks the same functions over heap buffers of exactly the sizes the kernels are promised -- the form the
// address and undefined-behaviour sanitizers run.
#include <stdint.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include "../../milagro_bls_amd/csrc/mbls_cmt.h"
#include "../../milagro_bls_amd/csrc/mbls_batch.h"

extern "C" {
int ch_route(uint32_t m, uint32_t s, int eligible, int mode) { return cmt_route(m, s, eligible, mode); }
uint32_t ch_count(const uint32_t* words, uint32_t m) { return cmt_count_selected(words, m); }
// the item's list as the wave writes it (positions j where members is null); list: m entries
uint32_t ch_expand(const uint32_t* words, const uint32_t* members, uint32_t m, int eligible, int mode, uint32_t* list, int* complement) {
    return cmt_expand_item(words, members, m, eligible, mode, list, complement);
}
// a committee batch built by the header's makers from addresses the caller chose (nothing is dereferenced), sliced, every per-item pointer read back
struct ch_flat { uint64_t sigs, results, bitmap, status, n, cmt_idx, bits, bits_stride, msg_idx, crecs, members, cmax, ccount, committee, indexed, key_idx, key_off; };
void ch_slice(const ch_flat* in, uint64_t lo, uint64_t hi, ch_flat* out) {
    batch b;
    b.d_sigs = (const uint8_t*)(uintptr_t)in->sigs; b.d_results = (uint8_t*)(uintptr_t)in->results; b.d_bitmap = (uint64_t*)(uintptr_t)in->bitmap;
    b.d_status = (uint32_t*)(uintptr_t)in->status; b.n = in->n; b.k = 0;
    b.ks = keys_committee(keys_table(nullptr, 0, nullptr, nullptr, nullptr), (const uint32_t*)(uintptr_t)in->crecs, in->ccount, (const uint32_t*)(uintptr_t)in->members,
                          (uint32_t)in->cmax, (const uint32_t*)(uintptr_t)in->cmt_idx, (const uint8_t*)(uintptr_t)in->bits, (uint32_t)in->bits_stride, nullptr);
    b.ms = msgs_table(nullptr, 0, nullptr, 0, (const uint32_t*)(uintptr_t)in->msg_idx);
    const batch t = slice(b, lo, hi);
    out->sigs = (uint64_t)(uintptr_t)t.d_sigs; out->results = (uint64_t)(uintptr_t)t.d_results; out->bitmap = (uint64_t)(uintptr_t)t.d_bitmap;
    out->status = (uint64_t)(uintptr_t)t.d_status; out->n = t.n; out->cmt_idx = (uint64_t)(uintptr_t)t.ks.d_cmt_idx; out->bits = (uint64_t)(uintptr_t)t.ks.d_bits;
    out->bits_stride = t.ks.bits_stride; out->msg_idx = (uint64_t)(uintptr_t)t.ms.d_idx; out->crecs = (uint64_t)(uintptr_t)t.ks.d_crecs;
    out->members = (uint64_t)(uintptr_t)t.ks.d_members; out->cmax = t.ks.cmax; out->ccount = t.ks.ccount; out->committee = t.ks.committee; out->indexed = t.ks.indexed;
    out->key_idx = (uint64_t)(uintptr_t)t.ks.d_idx; out->key_off = (uint64_t)(uintptr_t)t.ks.d_off;
}
}

#ifdef MBLS_CMT_HARNESS_MAIN
// every committee size 1 .. 130, 2047 and 2048, seeded bitfields and the all-ones field with stray bits, the three modes, eligible and not: the bitfield has exactly
// ceil(m / 32) words and the list exactly m entries, so a read or a write past either is the sanitizer's
static uint32_t rnd_state = 12345u;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 4; }
int main() {
    long checked = 0;
    for (uint32_t m = 1; m <= 2048; m = (m == 130 ? 2047 : m + 1)) {
        const uint32_t nw = (m + 31) / 32;
        for (int fill = 0; fill < 4; fill++) {
            uint32_t* words = (uint32_t*)malloc(4 * nw); uint32_t* list = (uint32_t*)malloc(4 * m); uint32_t* members = (uint32_t*)malloc(4 * m);
            for (uint32_t w = 0; w < nw; w++) words[w] = fill == 0 ? 0xFFFFFFFFu : fill == 1 ? 0u : fill == 2 ? rnd() * 16u + (rnd() & 15u) : ~(1u << (rnd() & 31u));
            for (uint32_t j = 0; j < m; j++) members[j] = 1000u + 7u * j;
            uint32_t s = 0;
            for (uint32_t j = 0; j < m; j++) s += (words[j >> 5] >> (j & 31)) & 1u;
            if (cmt_count_selected(words, m) != s) { printf("count m=%u\n", m); return 1; }
            for (int mode = 0; mode < 3; mode++) for (int el = 0; el < 2; el++) {
                int comp = -1; const uint32_t cnt = cmt_expand_item(words, members, m, el, mode, list, &comp);
                const int want_comp = el && mode != 1 && (mode == 2 || (uint64_t)(m - s) + 1 < s);
                if (comp != want_comp || cnt != (comp ? m - s : s)) { printf("route m=%u s=%u mode=%d el=%d\n", m, s, mode, el); return 1; }
                uint32_t at = 0;
                for (uint32_t j = 0; j < m; j++) {
                    const int sel = (words[j >> 5] >> (j & 31)) & 1u;
                    if (sel != comp) { if (list[at] != members[j]) { printf("list m=%u at=%u\n", m, at); return 1; } at++; }
                }
                checked++;
            }
            free(words); free(list); free(members);
        }
    }
    // a slice of a committee batch advances the two per-item pointers and nothing of the table
    ch_flat f; memset(&f, 0, sizeof(f)); ch_flat o;
    f.sigs = 1 << 20; f.results = 2 << 20; f.bitmap = 3 << 20; f.status = 4 << 20; f.n = 300; f.cmt_idx = 5 << 20; f.bits = 6 << 20; f.bits_stride = 20; f.msg_idx = 7 << 20;
    f.crecs = 8 << 20; f.members = 9 << 20; f.cmax = 129; f.ccount = 18;
    ch_slice(&f, 64, 300, &o);
    if (o.cmt_idx != f.cmt_idx + 4 * 64 || o.bits != f.bits + 20 * 64 || o.crecs != f.crecs || o.members != f.members || o.n != 236 || !o.committee) { printf("slice\n"); return 1; }
    printf("ok %ld\n", checked);
    return 0;
}
#endif

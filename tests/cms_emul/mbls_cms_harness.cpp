// The arithmetic of committee spans on the host (milagro_bls_amd/csrc/mbls_cms.h) and the span kind of the batch description (mbls_batch.h):
// tests/test_committee_span_cpu.py loads this file as a shared library and compares the two lists, the counts, the mask and the slices with a Python model. Built
// with -DMBLS_CMS_HARNESS_MAIN it is a program of its own that walks the same functions over heap buffers of exactly the sizes the kernels are promised -- the form
// the address and undefined-behaviour sanitizers run.
#include <stdint.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include "../../milagro_bls_amd/csrc/mbls_cms.h"
#include "../../milagro_bls_amd/csrc/mbls_batch.h"

extern "C" {
uint32_t sh_seg_offset(const uint32_t* sizes, uint32_t t) { return cms_seg_offset(sizes, t); }
uint32_t sh_count(const uint32_t* words, uint32_t o, uint32_t m) { return cms_count_selected(words, o, m); }
int sh_selected(const uint32_t* words, uint32_t o, uint32_t j) { return cms_selected(words, o, j); }
uint64_t sh_stride(uint32_t bits_stride, uint32_t max_members) { return cms_stride(bits_stride, max_members); }
int sh_range_ok(uint32_t lo, uint32_t hi, uint64_t n_ids, uint32_t* q) { return cms_range_ok(lo, hi, n_ids, q); }
// the item's region and record as the wave writes them (bit positions where members is null); region: stride words, rec: MBLS_CMS_REC_DWORDS
void sh_expand(const uint32_t* words, const uint32_t* members, const uint32_t* sizes, const uint32_t* firsts, const uint8_t* eligible, uint32_t q, int mode,
               uint32_t* region, uint64_t stride, uint32_t* rec) {
    cms_expand_item(words, members, sizes, firsts, eligible, q, mode, region, stride, rec);
}
int sh_plan(const uint32_t* sizes, const uint8_t* eligible, uint32_t q, const uint8_t* bits, uint32_t bits_bytes, int mode, uint64_t* mask, uint32_t* nd, uint32_t* nm) {
    return cms_plan_item(sizes, eligible, q, bits, bits_bytes, mode, mask, nd, nm);
}
// a span batch built by the header's makers from addresses the caller chose (nothing is dereferenced), sliced, every per-item pointer read back
struct sh_flat { uint64_t sigs, results, bitmap, status, n, cmt_idx, bits, bits_stride, msg_idx, crecs, members, cmax, ccount, committee, indexed, key_idx, key_off,
                 span, cmt_ids, n_cmt_ids, span_off; };
void sh_slice(const sh_flat* in, uint64_t lo, uint64_t hi, sh_flat* out) {
    batch b;
    b.d_sigs = (const uint8_t*)(uintptr_t)in->sigs; b.d_results = (uint8_t*)(uintptr_t)in->results; b.d_bitmap = (uint64_t*)(uintptr_t)in->bitmap;
    b.d_status = (uint32_t*)(uintptr_t)in->status; b.n = in->n; b.k = 0;
    b.ks = keys_committee_span(keys_table(nullptr, 0, nullptr, nullptr, nullptr), (const uint32_t*)(uintptr_t)in->crecs, in->ccount, (const uint32_t*)(uintptr_t)in->members,
                               (uint32_t)in->cmax, (const uint32_t*)(uintptr_t)in->cmt_ids, in->n_cmt_ids, (const uint32_t*)(uintptr_t)in->span_off,
                               (const uint8_t*)(uintptr_t)in->bits, (uint32_t)in->bits_stride, nullptr);
    b.ms = msgs_table(nullptr, 0, nullptr, 0, (const uint32_t*)(uintptr_t)in->msg_idx);
    const batch t = slice(b, lo, hi);
    out->sigs = (uint64_t)(uintptr_t)t.d_sigs; out->results = (uint64_t)(uintptr_t)t.d_results; out->bitmap = (uint64_t)(uintptr_t)t.d_bitmap;
    out->status = (uint64_t)(uintptr_t)t.d_status; out->n = t.n; out->cmt_idx = (uint64_t)(uintptr_t)t.ks.d_cmt_idx; out->bits = (uint64_t)(uintptr_t)t.ks.d_bits;
    out->bits_stride = t.ks.bits_stride; out->msg_idx = (uint64_t)(uintptr_t)t.ms.d_idx; out->crecs = (uint64_t)(uintptr_t)t.ks.d_crecs;
    out->members = (uint64_t)(uintptr_t)t.ks.d_members; out->cmax = t.ks.cmax; out->ccount = t.ks.ccount; out->committee = t.ks.committee; out->indexed = t.ks.indexed;
    out->key_idx = (uint64_t)(uintptr_t)t.ks.d_idx; out->key_off = (uint64_t)(uintptr_t)t.ks.d_off;
    out->span = t.ks.span; out->cmt_ids = (uint64_t)(uintptr_t)t.ks.d_cmt_ids; out->n_cmt_ids = t.ks.n_cmt_ids; out->span_off = (uint64_t)(uintptr_t)t.ks.d_cmt_span_off;
}
}

#ifdef MBLS_CMS_HARNESS_MAIN
// spans of 1, 2, 3 and 64 segments drawn from the edge sizes, seeded fields and the extreme ones, three modes, eligible and ineligible segments mixed. The field has
// exactly ceil(M / 32) words, the region exactly max(M, 1) words and the member array exactly M entries, so a read or a write past any of them is the sanitizer's.
static uint32_t rnd_state = 24680u;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 4; }
static const uint32_t EDGE[] = {1, 31, 32, 33, 63, 64, 65, 2048};
static int check_item(const uint32_t* sizes, const uint8_t* el, uint32_t q, int fill, int mode, long* checked) {
    uint32_t M = 0; uint32_t firsts[64];
    for (uint32_t t = 0; t < q; t++) { firsts[t] = M; M += sizes[t]; }
    const uint32_t nw = (M + 31) / 32; const uint64_t stride = M ? M : 1;
    uint32_t* words = (uint32_t*)malloc(4 * (nw ? nw : 1)); uint32_t* region = (uint32_t*)malloc(4 * stride); uint32_t* members = (uint32_t*)malloc(4 * (M ? M : 1));
    for (uint32_t w = 0; w < nw; w++) words[w] = fill == 0 ? 0xFFFFFFFFu : fill == 1 ? 0u : fill == 2 ? rnd() * 16u + (rnd() & 15u) : ~(1u << (rnd() & 31u));
    for (uint32_t j = 0; j < M; j++) members[j] = 1000u + 7u * j;
    for (uint64_t j = 0; j < stride; j++) region[j] = 0xDEADBEEFu;
    uint32_t rec[MBLS_CMS_REC_DWORDS];
    cms_expand_item(words, members, sizes, firsts, el, q, mode, region, stride, rec);
    uint32_t nd = 0, nm = 0, o = 0, total = 0; uint64_t mask = 0; int bad = 0;
    for (uint32_t t = 0; t < q && !bad; t++) {
        uint32_t s = 0;
        for (uint32_t j = 0; j < sizes[t]; j++) s += (words[(o + j) >> 5] >> ((o + j) & 31)) & 1u;
        if (cms_count_selected(words, o, sizes[t]) != s || cms_seg_offset(sizes, t) != o) { printf("count q=%u t=%u\n", q, t); bad = 1; break; }
        const int comp = el[t] && mode != 1 && (mode == 2 || (uint64_t)(sizes[t] - s) + 1 < s);
        for (uint32_t j = 0; j < sizes[t]; j++) {
            const int sel = (words[(o + j) >> 5] >> ((o + j) & 31)) & 1u;
            if (sel == comp) continue;
            const uint32_t got = comp ? region[stride - 1 - nm++] : region[nd++];
            if (got != members[o + j]) { printf("list q=%u t=%u j=%u\n", q, t, j); bad = 1; break; }
        }
        if (comp) mask |= 1ull << t;
        total += s; o += sizes[t];
    }
    if (!bad && (rec[0] != nd || rec[1] != nm || rec[2] != (uint32_t)mask || rec[3] != (uint32_t)(mask >> 32) || rec[4] != (total == 0 ? 1u : 0u))) { printf("rec q=%u\n", q); bad = 1; }
    for (uint64_t j = nd; !bad && j + nm < stride; j++) if (region[j] != 0xDEADBEEFu) { printf("written between the lists q=%u\n", q); bad = 1; }
    // the pure plan from the same field read as bytes
    uint64_t pmask = 0; uint32_t pnd = 0, pnm = 0;
    if (!bad && (cms_plan_item(sizes, el, q, (const uint8_t*)words, 4 * nw, mode, &pmask, &pnd, &pnm) != 0 || pmask != mask || pnd != nd || pnm != nm)) { printf("plan q=%u\n", q); bad = 1; }
    free(words); free(region); free(members);
    (*checked)++;
    return bad;
}
int main() {
    long checked = 0;
    uint32_t sizes[64]; uint8_t el[64];
    for (int fill = 0; fill < 4; fill++) for (int mode = 0; mode < 3; mode++) {
        for (uint32_t a = 0; a < 8; a++) for (int e = 0; e < 2; e++) { sizes[0] = EDGE[a]; el[0] = (uint8_t)e; if (check_item(sizes, el, 1, fill, mode, &checked)) return 1; }
        for (uint32_t a = 0; a < 8; a++) for (uint32_t b = 0; b < 8; b++) for (int e = 0; e < 4; e++) {
            sizes[0] = EDGE[a]; sizes[1] = EDGE[b]; el[0] = e & 1; el[1] = (e >> 1) & 1;
            if (check_item(sizes, el, 2, fill, mode, &checked)) return 1;
        }
        for (uint32_t a = 0; a < 7; a++) for (uint32_t b = 0; b < 7; b++) for (uint32_t c = 0; c < 8; c++) {
            sizes[0] = EDGE[a]; sizes[1] = EDGE[b]; sizes[2] = EDGE[c]; el[0] = 1; el[1] = (a + b) & 1; el[2] = 1;
            if (check_item(sizes, el, 3, fill, mode, &checked)) return 1;
        }
        for (int rep = 0; rep < 3; rep++) {
            for (uint32_t t = 0; t < 64; t++) { sizes[t] = rep == 2 ? 2048u : EDGE[rnd() % 7]; el[t] = (rnd() % 5) != 0; }
            if (check_item(sizes, el, 64, fill, mode, &checked)) return 1;
        }
        if (check_item(sizes, el, 0, fill, mode, &checked)) return 1;
    }
    // what the plan refuses
    uint64_t mk; uint32_t nd, nm; uint8_t field[8] = {0};
    sizes[0] = 64; el[0] = 1;
    if (cms_plan_item(sizes, el, 1, field, 8, 0, &mk, &nd, &nm) != 0 || cms_plan_item(sizes, el, 1, field, 7, 0, &mk, &nd, &nm) == 0 ||
        cms_plan_item(sizes, el, 65, field, 8, 0, &mk, &nd, &nm) == 0 || cms_plan_item(sizes, el, 1, field, 8, 3, &mk, &nd, &nm) == 0) { printf("plan refusals\n"); return 1; }
    sizes[0] = 0; if (cms_plan_item(sizes, el, 1, field, 8, 0, &mk, &nd, &nm) == 0) { printf("size 0\n"); return 1; }
    sizes[0] = 2049; if (cms_plan_item(sizes, el, 1, field, 8, 0, &mk, &nd, &nm) == 0) { printf("size 2049\n"); return 1; }
    // a slice of a span batch advances the offsets and the bits and nothing else of the key source
    sh_flat f; memset(&f, 0, sizeof(f)); sh_flat o;
    f.sigs = 1 << 20; f.results = 2 << 20; f.bitmap = 3 << 20; f.status = 4 << 20; f.n = 300; f.cmt_ids = 5 << 20; f.n_cmt_ids = 900; f.span_off = 10 << 20; f.bits = 6 << 20;
    f.bits_stride = 20; f.msg_idx = 7 << 20; f.crecs = 8 << 20; f.members = 9 << 20; f.cmax = 129; f.ccount = 18;
    sh_slice(&f, 64, 300, &o);
    if (o.span_off != f.span_off + 4 * 64 || o.bits != f.bits + 20 * 64 || o.cmt_ids != f.cmt_ids || o.n_cmt_ids != 900 || o.crecs != f.crecs || o.members != f.members ||
        o.n != 236 || !o.committee || !o.span || o.cmt_idx != 0) { printf("slice\n"); return 1; }
    printf("ok %ld\n", checked);
    return 0;
}
#endif

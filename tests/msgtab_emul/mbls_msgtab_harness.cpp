// mbls_msgtab_harness.cpp -- TEST INFRASTRUCTURE: the resident message table (include/mbls.h, mbls_msgtable_*) on the host. The table's index arithmetic
// (milagro_bls_amd/csrc/mbls_mtb.h: stride, entry of an index, growth, re-layout) with the lane bodies the HIP kernels wrap -- lane_h_export (k_h_export_tab) and
// lane_h_gather (k_h_gather) -- compiled as plain C++. The "hash" is a pattern: what is under test is where 72 dwords and a flag go and come back from, not their
// value. Not a fallback: the product library never loads this file.
#define MBLS_HOST_EMUL 1
#include <stdlib.h>
#include <string.h>
#include "../../milagro_bls_amd/csrc/mbls_ops.h"
#include "../../milagro_bls_amd/csrc/mbls_mtb.h"

struct mt_host {
    uint32_t *tab, *flags; uint64_t size, cap, growths;
};
static uint32_t pattern(uint32_t seed, int w) { return seed * 2654435761u + 0x9E3779B9u * (uint32_t)(w + 1); }
static void fill_h(mbls_ws& ws, uint64_t i, uint32_t seed) {
    for (int w = 0; w < MBLS_H_DWORDS; w++) ws.w[((uint64_t)MBLS_SLOT_H * 12 + w) * ws.stride + i] = pattern(seed, w);
}
static mbls_ws new_ws(uint64_t items) {
    mbls_ws ws; ws.stride = items; ws.w = (uint32_t*)calloc((size_t)MBLS_SLOT_COUNT * 12 * items, 4); return ws;
}
static void alloc_bufs(uint64_t cap, uint32_t** tab, uint32_t** flags) {
    *tab = (uint32_t*)malloc((size_t)MBLS_MTB_DWORDS * mtb_stride(cap) * 4); memset(*tab, 0xA5, (size_t)MBLS_MTB_DWORDS * mtb_stride(cap) * 4);
    *flags = (uint32_t*)malloc(mtb_stride(cap) * 4); memset(*flags, 0xA5, mtb_stride(cap) * 4);
}

extern "C" {
uint32_t mt_pattern(uint32_t seed, int w) { return pattern(seed, w); }
// the private entry (the empty message's) carries the pattern of empty_seed
void* mt_new(uint64_t capacity, uint32_t empty_seed) {
    mt_host* t = (mt_host*)calloc(1, sizeof(mt_host));
    t->cap = capacity; alloc_bufs(t->cap, &t->tab, &t->flags);
    mbls_ws ws = new_ws(1); uint32_t st = 0;
    fill_h(ws, 0, empty_seed);
    lane_h_export(ws, 0, t->tab, mtb_stride(t->cap), 0, t->flags, &st);
    free(ws.w); return t;
}
void mt_free(void* p) { mt_host* t = (mt_host*)p; free(t->tab); free(t->flags); free(t); }
uint64_t mt_size(void* p) { return ((mt_host*)p)->size; }
uint64_t mt_capacity(void* p) { return ((mt_host*)p)->cap; }
uint64_t mt_growths(void* p) { return ((mt_host*)p)->growths; }
// append n entries: message i has the pattern of seeds[i] and the status word st[i] of its own hash (its bad-range bit becomes the entry's flag) -> first index
uint64_t mt_append(void* p, uint64_t n, const uint32_t* seeds, const uint32_t* st) {
    mt_host* t = (mt_host*)p;
    const uint64_t ncap = mtb_grown(t->cap, t->size + n);
    if (ncap != t->cap) {
        uint32_t *nt, *nf; alloc_bufs(ncap, &nt, &nf);
        for (uint64_t e = 0; e <= t->size; e++) mtb_relayout_entry(t->tab, mtb_stride(t->cap), t->flags, nt, mtb_stride(ncap), nf, e);
        free(t->tab); free(t->flags); t->tab = nt; t->flags = nf; t->cap = ncap; t->growths++;
    }
    mbls_ws ws = new_ws(n ? n : 1);
    for (uint64_t i = 0; i < n; i++) fill_h(ws, i, seeds[i]);
    for (uint64_t i = 0; i < n; i++) lane_h_export(ws, i, t->tab, mtb_stride(t->cap), mtb_append_entry(t->size, i), t->flags, st);
    free(ws.w);
    const uint64_t first = t->size; t->size += n; return first;
}
// entry `e` (0: the private one; public index j: e = j + 1) read straight out of the buffers
void mt_read_entry(void* p, uint64_t e, uint32_t* out72, uint32_t* flag) {
    mt_host* t = (mt_host*)p;
    for (int w = 0; w < MBLS_MTB_DWORDS; w++) out72[w] = t->tab[mtb_at((uint64_t)w, mtb_stride(t->cap), e)];
    *flag = t->flags[e];
}
// what an item that names idx gets (lane_h_gather into workspace item `item` of `items`) -> the status bits the message brings
uint32_t mt_gather(void* p, uint32_t idx, uint64_t item, uint64_t items, uint32_t* out72) {
    mt_host* t = (mt_host*)p;
    mbls_ws ws = new_ws(items);
    const uint32_t st = lane_h_gather(ws, item, t->tab, mtb_stride(t->cap), t->flags, idx, t->size);
    for (int w = 0; w < MBLS_H_DWORDS; w++) out72[w] = ws.w[((uint64_t)MBLS_SLOT_H * 12 + w) * ws.stride + item];
    free(ws.w); return st;
}
uint64_t mt_entry_of(uint32_t idx, uint64_t size) { return mtb_entry(idx, size); }
}

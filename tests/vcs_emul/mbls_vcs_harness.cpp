// verify_multiple over committee spans on the host (milagro_bls_amd/csrc/mbls_vcs.h): tests/test_vm_committee_span_cpu.py loads this file as a shared library and
// compares the descriptor predicates, the expansion of a set, the chunk ranges and the split rule with a Python model. Built with -DMBLS_VCS_HARNESS_MAIN it is a
// program of its own that walks the same functions over heap buffers of exactly the sizes the kernels are promised -- the form the address and
// undefined-behaviour sanitizers run.
#include <stdint.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include "../../milagro_bls_amd/csrc/mbls_vcs.h"

extern "C" {
int vh_is_single(uint32_t q, uint32_t first_id) { return vcs_is_single(q, first_id); }
int vh_id_ok(uint32_t id, uint64_t ccount) { return vcs_id_ok(id, ccount); }
int vh_single_names_nothing(uint32_t id, uint64_t tsize) { return vcs_single_names_nothing(id, tsize); }
uint32_t vh_key_status(uint32_t st) { return vmc_key_status(st); }
// the set's region (`stride` words) and record as the wave leaves them -> 0 single-key, 1 expanded, 2 rejected
int vh_expand(uint32_t off_lo, uint32_t off_hi, const uint32_t* cmt_ids, uint64_t n_cmt_ids, const uint32_t* crecs, uint64_t ccount, const uint32_t* members,
              const uint32_t* words, uint32_t bits_stride, int mode, uint32_t* region, uint64_t stride, uint32_t* rec) {
    return vcs_expand_set(off_lo, off_hi, cmt_ids, n_cmt_ids, crecs, ccount, members, words, bits_stride, mode, region, stride, rec);
}
uint32_t vh_chunk_lo(uint32_t L, uint32_t P, uint32_t p) { return vcs_chunk_lo(L, P, p); }
uint64_t vh_lane_set(uint64_t g, uint32_t P) { return vcs_lane_set(g, P); }
uint32_t vh_lane_list(uint64_t g, uint32_t P) { return vcs_lane_list(g, P); }
uint32_t vh_lane_chunk(uint64_t g, uint32_t P) { return vcs_lane_chunk(g, P); }
uint64_t vh_lane_of(uint64_t i, uint32_t list, uint32_t p, uint32_t P) { return vcs_lane_of(i, list, p, P); }
uint64_t vh_extra_items(uint64_t n, uint32_t P) { return vcs_extra_items(n, P); }
int vh_split_mode_ok(int mode) { return vcs_split_mode_ok(mode); }
uint32_t vh_split(uint64_t n, uint64_t stride, uint64_t round_items, int mode) {
    mbls_limits L; memset(&L, 0, sizeof(L)); L.round_items = round_items;
    return vcs_split(n, stride, &L, mode);
}
uint32_t vh_split_max_sets(void) { return MBLS_VCS_SPLIT_MAX_SETS; }
uint32_t vh_min_chunk(void) { return MBLS_VCS_MIN_CHUNK; }
}

#ifdef MBLS_VCS_HARNESS_MAIN
// A table of committees of the edge sizes over a member array of exactly their total, id arrays of exactly the ids named, fields of exactly bits_stride bytes and
// regions of exactly cms_stride words: a read past any of them, or a write past the region or the record, is the sanitizer's.
static uint32_t rnd_state = 13579u;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 4; }
static const uint32_t EDGE[] = {1, 31, 32, 33, 63, 64, 65, 129};
#define NC 8u
int main() {
    uint32_t* crecs = (uint32_t*)calloc((size_t)MBLS_CMT_REC_DWORDS * NC, 4);
    uint32_t total = 0, cmax = 0;
    for (uint32_t c = 0; c < NC; c++) { crecs[MBLS_CMT_REC_DWORDS * c] = total; crecs[MBLS_CMT_REC_DWORDS * c + 1] = EDGE[c]; crecs[MBLS_CMT_REC_DWORDS * c + 2] = c != 3; total += EDGE[c]; if (EDGE[c] > cmax) cmax = EDGE[c]; }
    uint32_t* members = (uint32_t*)malloc(4 * total);
    for (uint32_t j = 0; j < total; j++) members[j] = 500u + 3u * j;
    long checked = 0;
    for (uint32_t bits_stride = 4; bits_stride <= 48; bits_stride += 44) for (int mode = 0; mode < 3; mode++) for (int rep = 0; rep < 400; rep++) {
        const uint64_t stride = cms_stride(bits_stride, cmax);
        uint32_t q = rep % 7 == 0 ? 65u : rep % 5 == 0 ? 1u : rnd() % 5u;
        uint32_t* ids = (uint32_t*)malloc(4 * (q ? q : 1));
        for (uint32_t t = 0; t < q; t++) ids[t] = rnd() % 11 == 0 ? NC + rnd() % 3u : rnd() % NC;
        if (q == 1 && rep % 2) ids[0] = MBLS_VMC_SINGLE_KEY | (rnd() % 200u);
        if (q >= 2 && rep % 9 == 0) ids[q - 1] = MBLS_VMC_SINGLE_KEY | 1u;
        uint32_t* words = (uint32_t*)malloc(bits_stride);
        for (uint32_t w = 0; w < bits_stride / 4; w++) words[w] = rnd() * 16u + (rnd() & 15u);
        uint32_t* region = (uint32_t*)malloc(4 * stride);
        uint32_t* rec = (uint32_t*)malloc(4 * MBLS_CMS_REC_DWORDS);
        for (uint64_t j = 0; j < stride; j++) region[j] = 0xDEADBEEFu;
        uint32_t lo = 0, hi = q; uint64_t n_ids = q;
        if (rep % 13 == 0) { lo = q; hi = 0; }                  // backwards (q > 0) or empty
        if (rep % 17 == 0) n_ids = q ? q - 1 : 0;               // past the ids
        const int kind = vcs_expand_set(lo, hi, ids, n_ids, crecs, NC, members, words, bits_stride, mode, region, stride, rec);
        // the model of the verdict
        int want = 1; uint64_t M = 0;
        if (hi < lo || hi > n_ids || hi - lo > 64u) want = 2;
        else if (hi - lo == 1 && (ids[lo] & MBLS_VMC_SINGLE_KEY)) want = 0;
        else {
            for (uint32_t t = lo; t < hi; t++) { if (ids[t] >= NC) { want = 2; break; } M += EDGE[ids[t]]; }
            if (want == 1 && M > 8u * bits_stride) want = 2;
        }
        if (kind != want) { printf("verdict rep=%d q=%u kind=%d want=%d\n", rep, q, kind, want); return 1; }
        if (kind == 0 && (region[0] != (ids[lo] & 0x7FFFFFFFu) || rec[0] != 1 || rec[1] || rec[2] || rec[3] || rec[4])) { printf("single\n"); return 1; }
        if (kind == 2 && (region[0] != 0xFFFFFFFFu || rec[0] != 1 || rec[1] || rec[2] || rec[3] || rec[4])) { printf("reject\n"); return 1; }
        if (kind != 1 && stride > 1 && region[1] != 0xDEADBEEFu) { printf("wrote past the one entry\n"); return 1; }
        if (kind == 1) {
            if ((uint64_t)rec[0] + rec[1] > M) { printf("counts\n"); return 1; }
            for (uint64_t j = rec[0]; j + rec[1] < stride; j++) if (region[j] != 0xDEADBEEFu) { printf("written between the lists\n"); return 1; }
            // every chunk of both lists under every factor lies inside its list, and the chunks tile it
            for (uint32_t P = 1; P <= MBLS_VCS_MAX_SPLIT; P *= 2) for (int which = 0; which < 2; which++) {
                const uint32_t L = rec[which ? 0 : 1];
                const uint32_t* first = region + (which || !L ? 0 : cms_missing_first(stride, L));
                uint32_t seen = 0, sum = 0;
                for (uint32_t p = 0; p < P; p++) {
                    const uint32_t a = vcs_chunk_lo(L, P, p), b = vcs_chunk_lo(L, P, p + 1);
                    if (a != seen || b < a || b > L) { printf("chunk L=%u P=%u p=%u\n", L, P, p); return 1; }
                    for (uint32_t j = a; j < b; j++) sum += first[j];
                    seen = b;
                }
                if (seen != L) { printf("tile L=%u P=%u\n", L, P); return 1; }
                (void)sum;
            }
        }
        free(ids); free(words); free(region); free(rec);
        checked++;
    }
    // lanes and sets
    for (uint32_t P = 1; P <= 16; P *= 2) for (uint64_t g = 0; g < 200; g++)
        if (vcs_lane_of(vcs_lane_set(g, P), vcs_lane_list(g, P), vcs_lane_chunk(g, P), P) != g) { printf("lane P=%u g=%lu\n", P, (unsigned long)g); return 1; }
    mbls_limits L; memset(&L, 0, sizeof(L)); L.round_items = 65536;
    for (uint64_t n = 1; n < 70000; n += 97) for (int mode = 0; mode <= 16; mode = mode ? mode * 2 : 1) {
        const uint32_t P = vcs_split(n, 8192, &L, mode);
        if (P < 1 || P > 16 || (P & (P - 1)) || (P > 1 && 2ull * P * n > L.round_items) || (!mode && 2 * n >= L.round_items && P != 1)) { printf("split n=%lu mode=%d\n", (unsigned long)n, mode); return 1; }
    }
    free(crecs); free(members);
    printf("ok %ld\n", checked);
    return 0;
}
#endif

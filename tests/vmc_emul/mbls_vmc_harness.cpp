// The set descriptor of mbls_verify_multiple_committee_msgtable* on the host (milagro_bls_amd/csrc/mbls_vmc.h, the functions k_vmc_expand runs): a program of its
// own that tests/test_vm_committee_cpu.py builds with -fsanitize=address,undefined, feeds a committee table and a list of sets on standard input, and compares
// with a Python restatement. Every buffer is a heap block of exactly the promised size -- a committee set's bitfield ceil(m / 32) words, its list m entries, a
// single-key set's list one entry and NO bitfield at all (a null pointer) -- so a read or a write past any of them, or a read of a single-key set's bits, ends
// the program.
//
// input:   C tsize                             committees, and the size of the key table (what the host entries refuse is judged against both)
//          m eligible                          C lines; committee c has members 1000 c + 7 j (j < m), laid back to back behind three words of padding
//          S                                   sets
//          word mode hexbits                   S lines; hexbits: the bitfield, 4 ceil(m / 32) bytes, or "-" (a set that has none)
// output:  single key_index names_nothing count route list...      one line per set
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../milagro_bls_amd/csrc/mbls_vmc.h"

int main() {
    unsigned long C = 0, S = 0, tsize = 0;
    if (scanf("%lu %lu", &C, &tsize) != 2) return 2;
    uint32_t* crecs = (uint32_t*)calloc(C ? C * MBLS_CMT_REC_DWORDS : 1, 4);
    std::vector<uint32_t> flat(3, 0xDEADu);
    for (unsigned long c = 0; c < C; c++) {
        unsigned m = 0, el = 0;
        if (scanf("%u %u", &m, &el) != 2 || m == 0 || m > MBLS_CMT_MAX_MEMBERS) return 2;
        uint32_t* rec = crecs + MBLS_CMT_REC_DWORDS * c;
        rec[0] = (uint32_t)flat.size(); rec[1] = m; rec[2] = el;
        for (unsigned j = 0; j < m; j++) flat.push_back((uint32_t)(1000u * c + 7u * j));
    }
    uint32_t* members = (uint32_t*)malloc(4 * flat.size());
    memcpy(members, flat.data(), 4 * flat.size());
    if (scanf("%lu", &S) != 1) return 2;
    static char hex[2 * 4 * (MBLS_CMT_MAX_MEMBERS / 32) + 8];
    for (unsigned long i = 0; i < S; i++) {
        unsigned long word = 0; int mode = 0;
        if (scanf("%lu %d %519s", &word, &mode, hex) != 3) return 2;
        const uint32_t w = (uint32_t)word;
        const bool committee = !vmc_is_single(w) && (uint64_t)w < C;
        const uint32_t m = committee ? crecs[MBLS_CMT_REC_DWORDS * w + 1] : 1u;
        uint32_t* words = nullptr;
        if (strcmp(hex, "-") != 0) {
            const size_t nb = strlen(hex) / 2;
            if (committee && nb != 4u * ((m + 31u) / 32u)) return 3;
            words = (uint32_t*)malloc(nb ? nb : 1);
            for (size_t b = 0; b < nb; b++) { unsigned v = 0; sscanf(hex + 2 * b, "%2x", &v); ((uint8_t*)words)[b] = (uint8_t)v; }
        } else if (committee) return 3;
        uint32_t* list = (uint32_t*)malloc(4 * m);
        uint32_t route = 0xFFFFFFFFu;
        const uint32_t cnt = vmc_expand_set(w, crecs, C, members, words, mode, list, &route);
        if (cnt > m) return 4;
        printf("%d %u %d %u %u", vmc_is_single(w), vmc_key_index(w), vmc_names_nothing(w, C, tsize), cnt, route);
        for (uint32_t t = 0; t < cnt; t++) printf(" %u", list[t]);
        printf("\n");
        free(list); free(words);
    }
    free(members); free(crecs);
    return 0;
}

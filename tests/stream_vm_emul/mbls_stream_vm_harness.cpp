// Host build of the verify_multiple stream's pure parts (milagro_bls_amd/csrc/mbls_stream.h): the whole-call rule the launcher cuts rounds with
// (stream_vm_fits, stream_take_whole, stream_vm_full), the ragged batch table of a round (stream_vm_offsets) and the destination dwords of the gather
// (stream_bits_fast, stream_bits_dword -- the text k_stream_gather_vm runs per dword, bits_len = 0 and a null source included). As a shared library for
// tests/test_stream_vm_cpu.py (svh_*), and with -DMBLS_STREAM_VM_HARNESS_MAIN a program of its own for the address and undefined-behaviour sanitizers: every
// source field then lies in a heap block of exactly misalignment + bits_len bytes, so a read outside [0, bits_len) of a field aborts the program.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../milagro_bls_amd/csrc/mbls_stream.h"

extern "C" {

int svh_fits(uint64_t round_items, uint64_t n_sets) { mbls_stream_opts o{}; o.round_items = round_items; return stream_vm_fits(o, n_sets); }

// the launcher's walk over a queue of calls (stream_walk under the whole-call rule, the step absorb runs): call j joins the open round or closes it; a launch is
// forced after call j where flush_after[j] != 0. out_round[j], out_first[j]: the round of call j and its first set there; out_batch[j]: its batch of the round.
// Returns the rounds, or -1 for a call that is refused at submit.
int64_t svh_walk(uint64_t round_items, const uint64_t* call_sets, const uint32_t* flush_after, uint64_t n_calls, uint64_t* out_round, uint64_t* out_first, uint64_t* out_batch) {
    mbls_stream_opts o{}; o.round_items = round_items;
    for (uint64_t j = 0; j < n_calls; j++) if (!stream_vm_fits(o, call_sets[j])) return -1;
    bool bad = false;
    const int64_t rounds = stream_walk(o, 1, n_calls,
        [&](uint64_t j) { return mbls_stream_call_shape{call_sets[j], 0, 4, nullptr, nullptr, flush_after ? flush_after[j] : 0u}; },
        [&](uint64_t j, uint64_t first, const mbls_stream_step& st, uint64_t round, const mbls_stream_fill& f) {
            out_round[j] = round; out_first[j] = st.round_first; out_batch[j] = st.batch;
            if (first || st.items != call_sets[j] || f.cost > round_items || f.cost != f.sets + f.calls) bad = true;
        });
    return rounds < 0 ? -2 : bad ? -3 : rounds;
}

void svh_offsets(const uint64_t* call_sets, uint64_t n_calls, uint32_t* off) { stream_vm_offsets(call_sets, n_calls, off); }

// what k_stream_gather_vm does with a tile's fields: `items` fields of bits_len bytes back to back at `bits` (bits_len = 0: bits may be null, nothing is read),
// out: items x bits_stride bytes (bits_stride a multiple of 4), every dword of it written; the fast decision is taken once, from the tile's first field
void svh_tile(const uint8_t* bits, uint32_t bits_len, uint32_t items, uint32_t bits_stride, uint32_t* out) {
    const uint32_t dpi = bits_stride / 4;
    const int fast = stream_bits_fast(bits, bits_len);
    for (uint64_t w = 0; w < (uint64_t)items * dpi; w++) {
        const uint64_t i = w / dpi;
        out[w] = stream_bits_dword(bits_len ? bits + (uint64_t)bits_len * i : bits, bits_len, (uint32_t)(w - i * dpi), fast);
    }
}

}  // extern "C"

#ifdef MBLS_STREAM_VM_HARNESS_MAIN
int main() {
    unsigned long checked = 0;
    uint32_t seed = 4242;
    auto next = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    const uint32_t stride = 20, lens[] = {0, 1, 3, 4, 17, stride};
    for (uint32_t bits_len : lens)
        for (uint32_t mis = 0; mis < 4; mis++)
            for (uint32_t items = 1; items <= 3; items++) {
                const size_t total = (size_t)bits_len * items;
                uint8_t* block = total ? (uint8_t*)malloc(mis + total) : nullptr;       // the fields start `mis` bytes in and end with the block
                uint8_t* bits = block ? block + mis : nullptr;
                for (size_t b = 0; b < total; b++) bits[b] = (uint8_t)next() | 1;
                uint32_t* out = (uint32_t*)malloc((size_t)stride * items);
                memset(out, 0xA5, (size_t)stride * items);
                svh_tile(bits, bits_len, items, stride, out);
                const uint8_t* ob = (const uint8_t*)out;
                for (uint32_t i = 0; i < items; i++)
                    for (uint32_t b = 0; b < stride; b++) {
                        const uint8_t want = b < bits_len ? bits[(size_t)bits_len * i + b] : 0;
                        if (ob[(size_t)stride * i + b] != want) { printf("FAIL bits_len %u mis %u items %u item %u byte %u\n", bits_len, mis, items, i, b); return 1; }
                        checked++;
                    }
                free(out); free(block);
            }
    // the walk and the offset tables over random queues, every array exactly as long as it is used
    for (int trial = 0; trial < 200; trial++) {
        const uint64_t R = 2 + next() % 40, n = 1 + next() % 30;
        uint64_t* sets = (uint64_t*)malloc(8 * n); uint32_t* fl = (uint32_t*)malloc(4 * n);
        uint64_t *rd = (uint64_t*)malloc(8 * n), *fs = (uint64_t*)malloc(8 * n), *bt = (uint64_t*)malloc(8 * n);
        for (uint64_t j = 0; j < n; j++) { sets[j] = 1 + next() % (R - 1); fl[j] = next() % 5 == 0; }
        const int64_t rounds = svh_walk(R, sets, fl, n, rd, fs, bt);
        if (rounds < 1) { printf("FAIL walk %d -> %lld\n", trial, (long long)rounds); return 1; }
        for (uint64_t j = 0; j < n;) {           // the table of each round: B + 1 words, the calls' first sets, then the round's sets
            uint64_t e = j; while (e < n && rd[e] == rd[j]) e++;
            const uint64_t B = e - j;
            uint32_t* off = (uint32_t*)malloc(4 * (B + 1));
            svh_offsets(sets + j, B, off);
            uint64_t sum = 0;
            for (uint64_t b = 0; b < B; b++) { if (off[b] != fs[j + b] || bt[j + b] != b) { printf("FAIL offsets %d\n", trial); return 1; } sum += sets[j + b]; checked++; }
            if (off[B] != sum || sum + B > R) { printf("FAIL round %d\n", trial); return 1; }
            free(off); j = e;
        }
        free(sets); free(fl); free(rd); free(fs); free(bt);
    }
    printf("ok %lu checks\n", checked);
    return 0;
}
#endif

// Host build of the committee stream's re-striding arithmetic (milagro_bls_amd/csrc/mbls_stream.h: stream_bits_fast, stream_bits_dword) -- the text
// k_stream_gather_cmt runs per destination dword. As a shared library for tests/test_stream_committee_cpu.py (sch_*), and with -DMBLS_STREAM_CMT_HARNESS_MAIN a
// program of its own for the address and undefined-behaviour sanitizers: every source field then lies in a heap block of exactly misalignment + bits_len bytes,
// so a read outside [0, bits_len) of the field aborts the program.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../milagro_bls_amd/csrc/mbls_stream.h"

extern "C" {

int sch_fast(const uint8_t* first_field, uint32_t bits_len) { return stream_bits_fast(first_field, bits_len); }

// one destination dword of one field
uint32_t sch_dword(const uint8_t* field, uint32_t bits_len, uint32_t j, int fast) { return stream_bits_dword(field, bits_len, j, fast); }

// what the kernel does with a tile: `items` fields of bits_len bytes back to back at `bits`, out: items x bits_stride bytes (bits_stride a multiple of 4),
// every dword of it written; the fast decision is taken once, from the tile's first field
void sch_tile(const uint8_t* bits, uint32_t bits_len, uint32_t items, uint32_t bits_stride, uint32_t* out) {
    const uint32_t dpi = bits_stride / 4;
    const int fast = stream_bits_fast(bits, bits_len);
    for (uint64_t w = 0; w < (uint64_t)items * dpi; w++) {
        const uint64_t i = w / dpi;
        out[w] = stream_bits_dword(bits + (uint64_t)bits_len * i, bits_len, (uint32_t)(w - i * dpi), fast);
    }
}

}  // extern "C"

#ifdef MBLS_STREAM_CMT_HARNESS_MAIN
int main() {
    unsigned long checked = 0;
    uint32_t seed = 12345;
    for (uint32_t bits_len = 1; bits_len <= 24; bits_len++)
        for (uint32_t mis = 0; mis < 4; mis++)
            for (uint32_t items = 1; items <= 3; items++) {
                // malloc returns 16-byte aligned blocks: the fields start `mis` bytes in and end with the block
                const size_t total = (size_t)bits_len * items;
                uint8_t* block = (uint8_t*)malloc(mis + total);
                uint8_t* bits = block + mis;
                for (size_t b = 0; b < total; b++) { seed = seed * 1664525u + 1013904223u; bits[b] = (uint8_t)(seed >> 24) | 1; }
                for (uint32_t stride = (bits_len + 3) / 4 * 4; stride <= 28; stride += 4) {
                    uint32_t* out = (uint32_t*)malloc((size_t)stride * items);
                    memset(out, 0xA5, (size_t)stride * items);
                    sch_tile(bits, bits_len, items, stride, out);
                    const uint8_t* ob = (const uint8_t*)out;
                    for (uint32_t i = 0; i < items; i++)
                        for (uint32_t b = 0; b < stride; b++) {
                            const uint8_t want = b < bits_len ? bits[(size_t)bits_len * i + b] : 0;
                            if (ob[(size_t)stride * i + b] != want) {
                                printf("FAIL bits_len %u mis %u items %u stride %u item %u byte %u\n", bits_len, mis, items, stride, i, b);
                                return 1;
                            }
                            checked++;
                        }
                    free(out);
                }
                free(block);
            }
    printf("ok %lu bytes\n", checked);
    return 0;
}
#endif

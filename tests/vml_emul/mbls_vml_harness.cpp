// mbls_vml_harness.cpp -- milagro_bls_amd/csrc/mbls_vml.h (the pure rules of mbls_verify_multiple_batches_locate*) built with the host compiler.
// "m": stdin "owned batch_ok status" per line -> "verdict status_out" (vml_mark: what k_vml_mark runs, one lane per set)
// "w": stdin "n B pair_hash" per line -> "shadow_first workspace_items flags_first" (what vmb_impl reserves and where the shadows and the flags lie)
#include <stdint.h>
#include <stdio.h>
#include "../../milagro_bls_amd/csrc/mbls_vml.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    unsigned long long a, b, c;
    if (argv[1][0] == 'm') {
        while (scanf("%llu %llu %llu", &a, &b, &c) == 3) {
            uint32_t st = 0;
            const uint32_t v = vml_mark(a != 0, b != 0, (uint32_t)c, &st);
            printf("%u %u\n", v, st);
        }
        return 0;
    }
    while (scanf("%llu %llu %llu", &a, &b, &c) == 3)
        printf("%llu %llu %llu\n", (unsigned long long)vml_shadow_first(a, b, c != 0), (unsigned long long)vml_workspace_items(a, b, c != 0),
               (unsigned long long)vml_flags_first(a, b));
    return 0;
}

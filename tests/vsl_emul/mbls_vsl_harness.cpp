// mbls_vsl_harness.cpp -- milagro_bls_amd/csrc/mbls_vsl.h (the pure rules of mbls_verify_multiple*_shared_msgs_locate*) built with the host compiler.
// "m": stdin "call_ok status msg_idx n_msgs flag_mask" per line -> "verdict status_out" (vsl_mark: what k_vsl_mark runs, one lane per set). The flags table
//      has n_msgs + 1 entries: entry 0 (the empty message's) carries a bit ON PURPOSE -- the rule must never read it for a listed message --, entry j + 1 is
//      the bad-range bit of message j, set where bit j of flag_mask is.
// "w": stdin "n n_msgs grouped list_items" per line -> "shadow_first workspace_items flags_first shadows_per_set"
// "s": stdin "t n" per line -> the set shadow item t answers for
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../../milagro_bls_amd/csrc/mbls_vsl.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    unsigned long long a, b, c, d, e;
    if (argv[1][0] == 'm') {
        while (scanf("%llu %llu %llu %llu %llu", &a, &b, &c, &d, &e) == 5) {
            std::vector<uint32_t> flags(d + 1, 0u);
            flags[0] = MBLS_VSL_BAD_MSG;
            for (unsigned long long j = 0; j < d && j < 64; j++) flags[j + 1] = ((e >> j) & 1) ? MBLS_VSL_BAD_MSG : 0u;
            uint32_t st = 0;
            const uint32_t v = vsl_mark(a != 0, (uint32_t)b, (uint32_t)c, d, flags.data(), &st);
            printf("%u %u\n", v, st);
        }
        return 0;
    }
    if (argv[1][0] == 's') {
        while (scanf("%llu %llu", &a, &b) == 2) printf("%llu\n", (unsigned long long)vsl_shadow_set(a, b));
        return 0;
    }
    while (scanf("%llu %llu %llu %llu", &a, &b, &c, &d) == 4)
        printf("%llu %llu %llu %llu\n", (unsigned long long)vsl_shadow_first(a, b, c != 0, d), (unsigned long long)vsl_workspace_items(a, b, c != 0, d),
               (unsigned long long)vsl_flags_first(a), (unsigned long long)vsl_shadows_per_set(c != 0));
    return 0;
}

// Host harness of milagro_bls_amd/csrc/mbls_vbg.h (tests/test_vm_batches_committee_cpu.py): the grouping of mbls_verify_multiple_batches_committee_msgtable*
// exactly as the kernels run it -- k_vmb_set_map's claims, then k_vbg_group's wave: 64 lanes per step, ballots, the lane walk, the scan of the sizes in steps of
// 64 groups --, the scan of the group counts, and the Miller items' rules (which batch a global group belongs to, overflow, live). The wave's result is also
// compared with the sequential statement vbg_group_batch.
// stdin, one case per line:  n T B spb max_groups  idx_0 .. idx_{n-1}  [off_0 .. off_B when spb = -1]
// stdout, per case, arrays separated by " | ":
//   pos | status | rlo | rhi | head | entry | count | goff | bound overflow_0 .. overflow_{B-1} | batch of group r for r < bound (-1: not live) | mismatches
//   mismatches: words in which the wave and vbg_group_batch differ, plus writes outside the batch's own range
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../milagro_bls_amd/csrc/mbls_vbg.h"

static uint32_t below(uint64_t mask, uint32_t lane) { return (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull)); }

struct arrays { std::vector<uint32_t> pos, rlo, rhi, head, entry, status; };

// k_vbg_group for one SOUND batch, lane by lane; `outside` counts writes that leave [lo, hi)
static uint32_t wave_group(const std::vector<uint32_t>& idx, uint64_t T, uint64_t lo, uint64_t hi, arrays& a, uint64_t& outside) {
    const uint32_t W = MBLS_VBG_WAVE;
    const uint64_t m = hi - lo;
    auto in = [&](uint64_t p) { if (p < lo || p >= hi) { outside++; return false; } return true; };
    uint32_t G = 0;
    if (!vbg_batch_grouped(m)) {
        for (uint64_t base = 0; base < m; base += W) {
            uint64_t mask = 0;
            for (uint32_t lane = 0; lane < W; lane++) { const uint64_t j = lo + base + lane; if (j < hi && vbg_valid(idx[j], T)) mask |= 1ull << lane; }
            for (uint32_t lane = 0; lane < W; lane++) {
                if (!((mask >> lane) & 1)) continue;
                const uint64_t j = lo + base + lane;
                const uint32_t g = G + below(mask, lane), p = (uint32_t)(lo + g);
                if (in(p)) { a.pos[j] = p; a.rlo[p] = p; a.rhi[p] = p + 1u; a.head[lo + g] = p; a.entry[lo + g] = idx[j]; }
            }
            G += (uint32_t)__builtin_popcountll(mask);
        }
        return G;
    }
    const uint32_t mm = (uint32_t)m;
    std::vector<uint32_t> s_idx(idx.begin() + lo, idx.begin() + hi), s_leader(mm), s_rank(mm), s_gnum(mm), s_size(mm), s_start(mm);
    for (uint32_t base = 0; base < mm; base += W) {
        uint64_t mask = 0;
        uint32_t l[64], r[64], sz[64]; bool v[64];
        for (uint32_t lane = 0; lane < W; lane++) {
            const uint32_t j = base + lane;
            l[lane] = MBLS_VBG_NONE; r[lane] = 0; sz[lane] = 0;
            v[lane] = j < mm && vbg_lane_walk(s_idx.data(), mm, j, T, &l[lane], &r[lane], &sz[lane]);
            if (v[lane] && l[lane] == j) mask |= 1ull << lane;
        }
        for (uint32_t lane = 0; lane < W; lane++) {
            const uint32_t j = base + lane;
            if (j < mm) { s_leader[j] = v[lane] ? l[lane] : MBLS_VBG_NONE; s_rank[j] = r[lane]; }
            if ((mask >> lane) & 1) { const uint32_t g = G + below(mask, lane); s_gnum[j] = g; s_size[g] = sz[lane]; if (in(lo + g)) a.entry[lo + g] = s_idx[j]; }
        }
        G += (uint32_t)__builtin_popcountll(mask);
    }
    uint32_t run = 0;
    for (uint32_t base = 0; base < G; base += W) {
        uint32_t incl[64], v[64];
        for (uint32_t lane = 0; lane < W; lane++) { const uint32_t g = base + lane; v[lane] = g < G ? s_size[g] : 0u; incl[lane] = v[lane]; }
        for (uint32_t d = 1; d < W; d *= 2) { uint32_t nx[64]; for (uint32_t lane = 0; lane < W; lane++) nx[lane] = incl[lane] + (lane >= d ? incl[lane - d] : 0u); for (uint32_t lane = 0; lane < W; lane++) incl[lane] = nx[lane]; }
        for (uint32_t lane = 0; lane < W; lane++) {
            const uint32_t g = base + lane; if (g >= G) continue;
            s_start[g] = run + incl[lane] - v[lane];
            if (in(lo + g)) a.head[lo + g] = (uint32_t)(lo + s_start[g]);
        }
        run += incl[W - 1];
    }
    for (uint32_t j = 0; j < mm; j++) {
        const uint32_t l = s_leader[j]; if (l == MBLS_VBG_NONE) continue;
        const uint32_t g = s_gnum[l], first = (uint32_t)(lo + s_start[g]), p = first + s_rank[j];
        if (in(p)) { a.pos[lo + j] = p; a.rlo[p] = first; a.rhi[p] = first + s_size[g]; }
    }
    return G;
}

static void put(const std::vector<uint32_t>& v) { for (uint32_t x : v) printf("%u ", x); printf("| "); }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        uint64_t n, T, B, max_groups; long long spb_in;
        in >> n >> T >> B >> spb_in >> max_groups;
        std::vector<uint32_t> idx(n), off;
        for (auto& x : idx) { uint64_t v; in >> v; x = (uint32_t)v; }
        const bool ragged = spb_in < 0;
        const uint32_t spb = ragged ? 0u : (uint32_t)spb_in;
        if (ragged) { off.resize(B + 1); for (auto& x : off) { uint64_t v; in >> v; x = (uint32_t)v; } }
        const uint32_t* po = ragged ? off.data() : nullptr;
        const uint64_t nn = n ? n : 1;
        // k_vmb_set_map
        std::vector<uint32_t> map(nn, MBLS_VMB_NO_OWNER);
        if (ragged)
            for (uint64_t b = 0; b < B; b++) {
                uint64_t lo, hi; if (!vmb_range(po, 0, n, b, &lo, &hi)) continue;
                for (uint64_t j = lo; j < hi; j++) map[j] = vmb_claim(map[j], (uint32_t)b);
            }
        arrays a, s;
        for (arrays* x : {&a, &s}) { x->pos.assign(nn, MBLS_VBG_NONE); x->rlo = x->rhi = x->head = x->entry = x->pos; x->status.assign(nn, 0); }
        std::vector<uint32_t> count(B, 0), scount(B, 0), goff(B + 1, 0);
        uint64_t outside = 0, mismatch = 0;
        for (uint64_t b = 0; b < B; b++) {
            uint64_t lo, hi;
            if (!vmb_range(po, spb, n, b, &lo, &hi)) continue;
            // the wave's first pass: the owned sets that name nothing are flagged whether or not the batch turns out sound
            for (uint64_t j = lo; j < hi; j++)
                if ((!ragged || map[j] == (uint32_t)b) && !vbg_valid(idx[j], T)) { a.status[j] |= MBLS_VBG_BAD_MSG; s.status[j] |= MBLS_VBG_BAD_MSG; }
            uint64_t lo2, hi2;
            if (!vbg_batch_sound(map.data(), po, spb, n, b, &lo2, &hi2)) continue;
            count[b] = wave_group(idx, T, lo, hi, a, outside);
            scount[b] = vbg_group_batch(idx.data(), T, lo, hi, s.pos.data(), s.rlo.data(), s.rhi.data(), s.head.data(), s.entry.data(), s.status.data());
        }
        for (uint64_t j = 0; j < n; j++)
            mismatch += (a.pos[j] != s.pos[j]) + (a.rlo[j] != s.rlo[j]) + (a.rhi[j] != s.rhi[j]) + (a.head[j] != s.head[j]) + (a.entry[j] != s.entry[j]) + (a.status[j] != s.status[j]);
        for (uint64_t b = 0; b < B; b++) { mismatch += count[b] != scount[b]; goff[b + 1] = goff[b] + count[b]; }
        a.pos.resize(n); a.rlo.resize(n); a.rhi.resize(n); a.head.resize(n); a.entry.resize(n); a.status.resize(n);
        put(a.pos); put(a.status); put(a.rlo); put(a.rhi); put(a.head); put(a.entry); put(count); put(goff);
        const uint64_t bound = vbg_bound(n, B, T, spb, max_groups, vbg_longest(n, spb, 0));
        printf("%llu ", (unsigned long long)bound);
        for (uint64_t b = 0; b < B; b++) printf("%d ", vbg_overflow(goff.data(), b, bound) ? 1 : 0);
        printf("| ");
        for (uint64_t r = 0; r < bound; r++) { uint64_t b = 0; printf("%lld ", vbg_group_live(goff.data(), B, bound, r, &b) ? (long long)b : -1ll); }
        printf("| %llu\n", (unsigned long long)(mismatch + outside));
    }
    return 0;
}

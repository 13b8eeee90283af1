// gather_cmt_probe.hip -- the one claim k_stream_gather_cmt makes: one round's gather of committee pieces through ONE record per tile,
// against the same round staged by FOUR k_stream_gather segments per piece (signatures, message indices, committee ids, fields -- possible only where bits_len
// equals the stride, which is what the comparison uses: 16-byte fields into a stride of 16). Pieces of 1 item and of 4 096 items, a round of 65 536 items;
// per variant the upload of the tile records from pinned memory plus the kernel, and the kernel alone, by HIP events; medians of REPS alternated repetitions, the
// staged bytes of both variants compared. The third variant is what only the new kernel can do: 17-byte fields at an odd address into a stride of 20.
// The kernels are the library's own text: this file includes csrc/mbls_stream.hip and links against the library for the entries that file calls.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -o scripts/dbg/gather_cmt_probe scripts/dbg/gather_cmt_probe.hip -Lmilagro_bls_amd -lmbls_hip
//        -Wl,-rpath,$PWD/milagro_bls_amd;  run: scripts/dbg/gather_cmt_probe [OUT.json]
#include "../../milagro_bls_amd/csrc/mbls_stream.hip"
#include <stdlib.h>

// the hooks below the ABI are not exported from the library; the probe never creates a stream
extern "C" void mblsi_msgtable_stream_calls(mbls_msgtable*, long long) {}
extern "C" void mblsi_committees_stream_calls(mbls_committees*, long long) {}
extern "C" int mblsi_committees_stream_bind(mbls_ctx*, mbls_committees*, uint32_t) { return MBLS_ERR_ARGUMENT; }
extern "C" void mblsi_committees_stream_unbind(mbls_committees*, uint32_t) {}

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)
static const uint64_t R = 65536;
static const int REPS = 21;

struct bufs { uint8_t *sigs, *bits, *o_sigs, *o_bits; uint32_t *midx, *cid, *o_midx, *o_cid; uint8_t *d_meta, *h_meta; };

static double median(std::vector<float>& v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

// -> {ms with upload, ms kernel alone}
template <typename F>
static void timed(const void* h, void* d, size_t bytes, F launch, hipStream_t s, float* with_upload, float* kernel) {
    hipEvent_t a, b, c; CHK(hipEventCreate(&a)); CHK(hipEventCreate(&b)); CHK(hipEventCreate(&c));
    CHK(hipEventRecord(a, s));
    CHK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s));
    CHK(hipEventRecord(b, s));
    launch();
    CHK(hipGetLastError());
    CHK(hipEventRecord(c, s));
    CHK(hipEventSynchronize(c));
    float up; CHK(hipEventElapsedTime(&up, a, b)); CHK(hipEventElapsedTime(kernel, b, c));
    *with_upload = up + *kernel;
    CHK(hipEventDestroy(a)); CHK(hipEventDestroy(b)); CHK(hipEventDestroy(c));
}

int main(int argc, char** argv) {
    FILE* out = argc > 1 ? fopen(argv[1], "w") : stdout;
    if (!out) return 1;
    hipStream_t s; CHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    bufs B{};
    const uint64_t MAXB = 20;
    CHK(hipMalloc(&B.sigs, 96 * R)); CHK(hipMalloc(&B.midx, 4 * R)); CHK(hipMalloc(&B.cid, 4 * R)); CHK(hipMalloc(&B.bits, MAXB * R + 16));
    CHK(hipMalloc(&B.o_sigs, 96 * R)); CHK(hipMalloc(&B.o_midx, 4 * R)); CHK(hipMalloc(&B.o_cid, 4 * R)); CHK(hipMalloc(&B.o_bits, MAXB * R));
    const size_t meta = 4 * (R + 64) * sizeof(gtile) + 1024;
    CHK(hipMalloc(&B.d_meta, meta)); CHK(hipHostMalloc((void**)&B.h_meta, meta, hipHostMallocDefault));
    {
        std::vector<uint8_t> h(96 * R + 8 * R + MAXB * R + 16);
        uint32_t x = 2463534242u;
        for (auto& v : h) { x ^= x << 13; x ^= x >> 17; x ^= x << 5; v = (uint8_t)x; }
        CHK(hipMemcpy(B.sigs, h.data(), 96 * R, hipMemcpyHostToDevice)); CHK(hipMemcpy(B.midx, h.data() + 96 * R, 4 * R, hipMemcpyHostToDevice));
        CHK(hipMemcpy(B.cid, h.data() + 100 * R, 4 * R, hipMemcpyHostToDevice)); CHK(hipMemcpy(B.bits, h.data() + 104 * R, MAXB * R + 16, hipMemcpyHostToDevice));
    }
    fprintf(out, "{\n \"what\": \"one round's gather of %llu committee items: tile records uploaded from pinned memory + kernel, and the kernel alone; HIP events, ms, median of %d "
                 "alternated repetitions\",\n \"rows\": {\n", (unsigned long long)R, REPS);
    const uint64_t piece_sizes[2] = {1, 4096};
    for (int pi = 0; pi < 2; pi++) {
        const uint64_t p = piece_sizes[pi];
        // four k_stream_gather segments per piece (16-byte fields into a stride of 16), cut as the launcher's seg() cuts them
        std::vector<gtile> gt;
        auto seg = [&](const uint8_t* src, uint8_t* dst, uint64_t bytes) { for (uint64_t o = 0; o < bytes; o += GATHER_TILE) gt.push_back(gtile{src + o, dst + o, std::min(GATHER_TILE, bytes - o)}); };
        std::vector<ctile> c16, c17;
        for (uint64_t a = 0; a < R; a += p) {
            seg(B.sigs + 96 * a, B.o_sigs + 96 * a, 96 * p);
            seg((const uint8_t*)(B.midx + a), (uint8_t*)(B.o_midx + a), 4 * p);
            seg((const uint8_t*)(B.cid + a), (uint8_t*)(B.o_cid + a), 4 * p);
            seg(B.bits + 16 * a, B.o_bits + 16 * a, 16 * p);
            for (uint64_t t = a; t < a + p; t += CMT_TILE) {
                const uint32_t items = (uint32_t)std::min(CMT_TILE, a + p - t);
                c16.push_back(ctile{B.sigs + 96 * t, B.midx + t, B.cid + t, B.bits + 16 * t, 16, items, t});
                c17.push_back(ctile{B.sigs + 96 * t, B.midx + t, B.cid + t, B.bits + 1 + 17 * t, 17, items, t});
            }
        }
        if (gt.size() * sizeof(gtile) > meta) return 2;
        std::vector<float> t4u, t4k, t1u, t1k, t17u, t17k;
        std::vector<uint8_t> want(120 * R), got(120 * R);
        auto snapshot = [&](std::vector<uint8_t>& v) {
            CHK(hipMemcpy(v.data(), B.o_sigs, 96 * R, hipMemcpyDeviceToHost)); CHK(hipMemcpy(v.data() + 96 * R, B.o_midx, 4 * R, hipMemcpyDeviceToHost));
            CHK(hipMemcpy(v.data() + 100 * R, B.o_cid, 4 * R, hipMemcpyDeviceToHost)); CHK(hipMemcpy(v.data() + 104 * R, B.o_bits, 12 * R + 4 * R, hipMemcpyDeviceToHost));
        };
        auto clear = [&] { CHK(hipMemset(B.o_sigs, 0xEE, 96 * R)); CHK(hipMemset(B.o_midx, 0xEE, 4 * R)); CHK(hipMemset(B.o_cid, 0xEE, 4 * R)); CHK(hipMemset(B.o_bits, 0xEE, MAXB * R)); };
        for (int r = 0; r < REPS + 2; r++) {
            float u, k;
            if (r == 0) clear();
            memcpy(B.h_meta, gt.data(), gt.size() * sizeof(gtile));
            timed(B.h_meta, B.d_meta, gt.size() * sizeof(gtile), [&] { hipLaunchKernelGGL(k_stream_gather, dim3((unsigned)gt.size()), dim3(SWG), 0, s, (const gtile*)B.d_meta); }, s, &u, &k);
            if (r >= 2) { t4u.push_back(u); t4k.push_back(k); }
            if (r == 0) { snapshot(want); clear(); }
            memcpy(B.h_meta, c16.data(), c16.size() * sizeof(ctile));
            timed(B.h_meta, B.d_meta, c16.size() * sizeof(ctile), [&] { hipLaunchKernelGGL(k_stream_gather_cmt, dim3((unsigned)c16.size()), dim3(SWG), 0, s, (const ctile*)B.d_meta, B.o_sigs, B.o_midx, B.o_cid, B.o_bits, 16u); }, s, &u, &k);
            if (r >= 2) { t1u.push_back(u); t1k.push_back(k); }
            if (r == 0) { snapshot(got); if (memcmp(want.data(), got.data(), 120 * R)) { fprintf(stderr, "the two variants staged different bytes (pieces of %llu)\n", (unsigned long long)p); return 3; } }
            memcpy(B.h_meta, c17.data(), c17.size() * sizeof(ctile));
            timed(B.h_meta, B.d_meta, c17.size() * sizeof(ctile), [&] { hipLaunchKernelGGL(k_stream_gather_cmt, dim3((unsigned)c17.size()), dim3(SWG), 0, s, (const ctile*)B.d_meta, B.o_sigs, B.o_midx, B.o_cid, B.o_bits, 20u); }, s, &u, &k);
            if (r >= 2) { t17u.push_back(u); t17k.push_back(k); }
        }
        fprintf(out, "  \"pieces_of_%llu\": {\"pieces\": %llu, \"four_segments\": {\"tiles\": %zu, \"record_bytes\": %zu, \"upload_and_kernel_ms\": %.4f, \"kernel_ms\": %.4f},\n"
                     "    \"gather_cmt_16_into_16\": {\"tiles\": %zu, \"record_bytes\": %zu, \"upload_and_kernel_ms\": %.4f, \"kernel_ms\": %.4f},\n"
                     "    \"gather_cmt_17_into_20_unaligned\": {\"tiles\": %zu, \"record_bytes\": %zu, \"upload_and_kernel_ms\": %.4f, \"kernel_ms\": %.4f}}%s\n",
                (unsigned long long)p, (unsigned long long)(R / p), gt.size(), gt.size() * sizeof(gtile), median(t4u), median(t4k), c16.size(), c16.size() * sizeof(ctile), median(t1u),
                median(t1k), c17.size(), c17.size() * sizeof(ctile), median(t17u), median(t17k), pi == 0 ? "," : "");
    }
    fprintf(out, " }\n}\n");
    if (out != stdout) fclose(out);
    return 0;
}

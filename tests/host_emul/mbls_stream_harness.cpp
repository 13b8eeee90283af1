// mbls_stream_harness.cpp -- TEST INFRASTRUCTURE: the pure parts of the verification stream (milagro_bls_amd/csrc/mbls_stream.h) built with the
// host compiler, so tests/test_stream_cpu.py can check the scatter's bit arithmetic and the layout decision of a round without a GPU.
#include "../../milagro_bls_amd/csrc/mbls_stream.h"

extern "C" {
// what k_stream_scatter does to the caller's bitmap for one piece: words entirely inside the piece stored whole, boundary words OR-ed in.
// Returns the number of words stored whole.
uint64_t harness_scatter_bits(const uint8_t* round_res, uint64_t round_first, uint64_t call_first, uint64_t items, uint64_t* bitmap) {
    uint64_t w0, nw, whole_words = 0; stream_bitmap_words(call_first, items, &w0, &nw);
    for (uint64_t j = 0; j < nw; j++) {
        int whole; const uint64_t bits = stream_bitmap_word(round_res, round_first, call_first, items, w0 + j, &whole);
        if (whole) { bitmap[w0 + j] = bits; whole_words++; }
        else bitmap[w0 + j] |= bits;
    }
    return whole_words;
}
// the layout decision of a round made of pieces of these calls (in order)
void harness_layout(const mbls_stream_call_shape* calls, uint64_t n, int* keys_uniform, int* msgs_uniform) {
    mbls_stream_layout l{};
    for (uint64_t i = 0; i < n; i++) stream_layout_add(l, i == 0, calls[i]);
    *keys_uniform = l.keys_uniform; *msgs_uniform = l.msgs_uniform;
}
}

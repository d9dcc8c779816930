// vfa_conv_grad.h -- the integer rules of the weight gradient of the dense 3x3 convolution (vfa_conv_grad.hip; host / device code;
// tests/native/conv_grad_harness.cpp checks them against a brute-force enumeration): how the cells of a map are cut into slabs, and
// where a partial sum lies in the workspace.
//
// The cells are the K dimension of the product.  They are walked in the forward kernel's tiles (vfa_conv.h: kTileRows x kTileCols
// cells, row-major over the map), and a SLAB is a run of consecutive tiles.  The cut is a function of (L, W) alone: a map of n
// tiles has min(n, kMaxSlabs) slabs and slab s owns the tiles [n s / slabs, n (s + 1) / slabs) -- never empty, every tile in
// exactly one slab -- so what is summed where depends on neither the device nor the batch.  A workgroup owns one (frame, slab) and
// one tile of kTileO outputs x kTileC inputs x 9 taps of the result and writes it, unscaled, as one float32 partial; the merge
// kernel adds the partials of an element in ascending (frame, slab) order.
#ifndef VFA_CONV_GRAD_H
#define VFA_CONV_GRAD_H
#include <stddef.h>

#include "vfa_conv.h"

namespace vfa_conv_grad {

constexpr int kTileO = 128;    // outputs of a workgroup's tile: one 32-row MFMA operand per wave
constexpr int kTileC = 32;     // inputs of a workgroup's tile: the chunk of vfa_conv.h
constexpr int kMaxSlabs = 16;  // slabs of a map
constexpr int kGHalves = kTileO + 8; // fp16 values per cell of the staged output gradient: 128 outputs + 8 of padding (272 bytes)

VFA_CONV_HD int tiles(int L, int W) { return vfa_conv::tiles_x(W) * vfa_conv::tiles_y(L); }
VFA_CONV_HD int slabs(int L, int W) { return tiles(L, W) < kMaxSlabs ? tiles(L, W) : kMaxSlabs; }
// first tile of slab s (s == slabs: one past the last tile)
VFA_CONV_HD int slab_begin(int s, int L, int W) { return (int)((long long)tiles(L, W) * s / slabs(L, W)); }

// floats of one (frame, slab) partial: laid out [tap][o][c], the whole (O, C) plane of every tap
VFA_CONV_HD size_t partial_floats(int O, int C) { return (size_t)vfa_conv::kTaps * (size_t)O * (size_t)C; }
// index of element (o, c, tap t) in the partial of (frame b, slab s)
VFA_CONV_HD size_t partial_index(int b, int s, int t, int o, int c, int O, int C, int L, int W)
{
    return ((size_t)b * slabs(L, W) + s) * partial_floats(O, C) + ((size_t)t * O + o) * C + c;
}

} // namespace vfa_conv_grad
#endif // VFA_CONV_GRAD_H

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
//
// The trunk's layers (vfa_trunk_conv_wgrad_f32) have up to 512 x 512 weights on small maps, where kMaxSlabs partials of 9 O C floats per
// frame are larger than the operands: slabs_for(L, W, O, C) is slabs(L, W) up to O C = 256^2 and shrinks in proportion past it (at
// least one), so a frame's partials never exceed those of a 256 x 256 layer on the same map -- a rule of the shape alone, too.  The
// forms that end in _of take the number of slabs; with slabs(L, W) they are the forms above.
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

// slabs of the trunk's weight gradient: slabs(L, W) wherever O C <= kFullSlabsOC, never more partial floats per frame than there
constexpr long long kFullSlabsOC = 256LL * 256;
VFA_CONV_HD int slabs_for(int L, int W, int O, int C)
{
    const long long oc = (long long)O * C;
    if (oc <= kFullSlabsOC) return slabs(L, W);
    const long long n = (long long)slabs(L, W) * kFullSlabsOC / oc;
    return n < 1 ? 1 : (int)n;
}
// first tile of slab s of n_slabs (1 <= n_slabs <= tiles; s == n_slabs: one past the last tile)
VFA_CONV_HD int slab_begin_of(int s, int n_slabs, int L, int W) { return (int)((long long)tiles(L, W) * s / n_slabs); }
VFA_CONV_HD size_t partial_index_of(int b, int s, int n_slabs, int t, int o, int c, int O, int C)
{
    return ((size_t)b * n_slabs + s) * partial_floats(O, C) + ((size_t)t * O + o) * C + c;
}

} // namespace vfa_conv_grad
#endif // VFA_CONV_GRAD_H

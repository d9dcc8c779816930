// vfa_decode.h -- the integer logic of the fused BEV decode (vfa_decode.hip) as plain host / device code: the 64-bit selection key,
// the radix select that finds the k-th largest key of a frame, and the bitonic network that orders the selected keys.  The kernel
// runs these functions from the threads of one workgroup; tests/native/decode_select_harness.cpp compiles this file with g++, runs
// the same functions from loops and checks the selection against std::sort.
//
// The problem: a frame of n_cells confidences; a CANDIDATE is a cell with conf > thresh (thresh >= 0, so a candidate's float bits
// are a positive integer that grows with the value); keep the k candidates that come first by confidence descending, equal
// confidences by ascending cell index, and list them in that order.
//
// The key: (float bits << 32) | (0xffffffff - cell).  Unique per cell, and "comes first" is exactly "has the larger key".  So the
// answer is the k largest keys in descending order, whatever the confidences are: a constant map gives the k lowest cells.
//
// The select: the k-th largest key, one 8-bit digit per pass from the top.  A pass counts, for every candidate whose known digits
// equal the prefix found so far, its digit into 256 bins; `select_advance` walks the bins from the top to the one that holds the
// k-th key, adds its digit to the prefix and lowers `need` by the keys of the bins above.  The passes are known beforehand: the four
// digits of the confidence and those digits of the cell index in which two cells of the frame can differ (`pass_counts`), eight at
// the most.  The select may end before the last of them, when every key of the bin is wanted (`done`): the threshold is then the
// prefix with zeros below it.  The selected keys are the candidates with key >= threshold: min(k, number of candidates) of them.
#ifndef VFA_DECODE_H
#define VFA_DECODE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define VFA_DECODE_HD __host__ __device__ __forceinline__
#else
#define VFA_DECODE_HD inline
#endif

namespace vfa_decode {

constexpr int kMaxTopk = 1024; // keys one workgroup orders in LDS (VFA_BEV_DECODE_MAX_TOPK of include/vfa_hip.h)
constexpr int kBins = 256;     // one 8-bit digit per pass
constexpr int kPasses = 8;     // digits of a key

VFA_DECODE_HD uint64_t pack_key(uint32_t conf_bits, uint32_t cell) { return ((uint64_t)conf_bits << 32) | (uint64_t)(0xffffffffu - cell); }
VFA_DECODE_HD uint32_t key_conf_bits(uint64_t key) { return (uint32_t)(key >> 32); }
VFA_DECODE_HD uint32_t key_cell(uint64_t key) { return 0xffffffffu - (uint32_t)key; }

VFA_DECODE_HD int pass_shift(int pass) { return 56 - 8 * pass; }
// pass 0..3: the confidence; pass 4..7: digit 3..0 of the cell index, counted only where two cells of the frame can differ in it
VFA_DECODE_HD bool pass_counts(int pass, long long n_cells)
{
    return pass < 4 || (((n_cells - 1) >> (8 * (7 - pass))) != 0);
}

struct Select {
    uint64_t prefix; // the digits of the k-th key found so far, zeros elsewhere
    uint64_t known;  // mask of those digits
    int need;        // how many keys that match the prefix are wanted, >= 1
    int done;        // prefix is the threshold
};

// every digit no pass counts is 0xff in every key (the inverted index of a cell below 2^(8 d) has all ones from digit d up)
VFA_DECODE_HD Select select_begin(int k, long long n_cells)
{
    Select s = {0, 0, k, 0};
    for (int pass = 4; pass < kPasses; ++pass)
        if (!pass_counts(pass, n_cells)) {
            s.prefix |= (uint64_t)0xff << pass_shift(pass);
            s.known |= (uint64_t)0xff << pass_shift(pass);
        }
    return s;
}

VFA_DECODE_HD bool select_matches(const Select &s, uint64_t key) { return (key & s.known) == s.prefix; }
VFA_DECODE_HD int key_digit(uint64_t key, int pass) { return (int)((key >> pass_shift(pass)) & 0xff); }

// hist[d] = number of candidates that match the prefix and have digit d in this pass.  Fewer matching keys than wanted (only the
// first pass can see that: fewer candidates than k): every candidate is selected.
VFA_DECODE_HD void select_advance(Select &s, const unsigned *hist, int pass)
{
    long long above = 0;
    int bin = -1;
    long long above_bin = 0;
    for (int d = kBins - 1; d >= 0; --d) { // (no early exit: 256 independent reads)
        const long long c = hist[d];
        if (bin < 0 && above + c >= s.need) { bin = d; above_bin = above; }
        above += c;
    }
    if (bin < 0 || above == s.need) { s.done = 1; return; } // all the matching keys are wanted: the threshold is the prefix
    s.prefix |= (uint64_t)bin << pass_shift(pass);
    s.known |= (uint64_t)0xff << pass_shift(pass);
    s.need -= (int)above_bin;
    if ((long long)hist[bin] == s.need) s.done = 1;
}

VFA_DECODE_HD bool select_takes(const Select &s, uint64_t key) { return key >= s.prefix; }

// Bitonic network, descending: for size = 2, 4 .. n and stride = size / 2 .. 1, exchange `t` of n / 2 (n a power of two) compares one
// pair; the exchanges of one (size, stride) touch disjoint pairs and may run in any order or at once.
VFA_DECODE_HD void bitonic_exchange(uint64_t *keys, int t, int size, int stride)
{
    const int i = 2 * t - (t & (stride - 1)), j = i + stride;
    const uint64_t a = keys[i], b = keys[j];
    const bool descending = (i & size) == 0;
    if ((a < b) == descending) { keys[i] = b; keys[j] = a; }
}
VFA_DECODE_HD int pow2_at_least(int n)
{
    int p = 1;
    for (int b = 0; b < 31 && p < n; ++b) p <<= 1;
    return p;
}

} // namespace vfa_decode
#endif // VFA_DECODE_H

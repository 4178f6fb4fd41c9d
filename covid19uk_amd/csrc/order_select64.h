// The 64-bit twin of order_select.h: one step of an MSB-first radix select over fp64 values, host + device (plain C++ for
// tests/test_rt_quantiles_host.py, __device__ for k_order_stats_f64 of order_stats64_kernels.h).
//
// The order is DEFINED as that of IEEE-754 totalOrder on the bit pattern: a value is compared through its key,
//   key = bits ^ (bits >> 63 ? ~0ull : 1ull << 63),
// as an unsigned 64-bit number (a negative value has all its bits flipped, a positive one its sign bit).  On arrays without
// NaN this is the order of np.sort, bit for bit, except that -0.0 sorts before +0.0 (np.sort leaves equal values in any
// order); NaNs sort by sign and payload, the negative ones before -inf and the positive ones behind +inf (np.sort puts every
// NaN last).  The key is cut into ORDER64_PASSES digits of ORDER_DIGIT_BITS bits, the most significant first.  A rank's state
// is (prefix, rank): the digits found so far, 64 bits, and the rank that remains among the values whose key starts with them,
// 32 bits; it starts as (0, r).  Pass p counts, for the values whose key agrees with the prefix on the digits above digit p,
// digit p into a histogram of ORDER_BINS bins; order64_select_narrow moves the state one digit down.  After the last pass the
// prefix IS the key of the r-th value in that order, and order64_value gives its bits back.  Everything is integer
// arithmetic and exact for any values and any n < 2^32.
#pragma once

#include "order_select.h"

namespace seir {

constexpr int ORDER64_PASSES = 64 / ORDER_DIGIT_BITS;

SEIR_OS_HD uint64_t order64_key(uint64_t bits) { return bits ^ ((bits >> 63) ? ~0ull : 1ull << 63); }
// the inverse: a key with its top bit set came from a positive value
SEIR_OS_HD uint64_t order64_value(uint64_t key) { return key ^ ((key >> 63) ? 1ull << 63 : ~0ull); }

// Bit position of digit `pass` (pass 0 is the most significant).
SEIR_OS_HD int order64_shift(int pass) { return 64 - ORDER_DIGIT_BITS * (pass + 1); }
// The digit of `key` that pass `pass` counts.
SEIR_OS_HD uint32_t order64_digit(uint64_t key, int pass) { return (uint32_t)(key >> order64_shift(pass)) & (uint32_t)(ORDER_BINS - 1); }
// Does `key` agree with `prefix` on every digit above digit `pass`?  (Always in pass 0.)
SEIR_OS_HD bool order64_matches(uint64_t key, uint64_t prefix, int pass) {
    return pass == 0 || ((key ^ prefix) >> (order64_shift(pass) + ORDER_DIGIT_BITS)) == 0ull;
}

// order_select_narrow's step with a 64-bit prefix: hist [ORDER_BINS] are the counts of digit `pass` among the values that
// match `prefix`; 0 <= rank < sum(hist).  The smallest digit d with hist[0] + .. + hist[d] > rank goes into the prefix, and
// rank becomes the rank among that bin's values.  Returns false, and leaves the state alone, if rank >= sum(hist).
SEIR_OS_HD bool order64_select_narrow(const uint32_t *hist, int pass, uint64_t &prefix, uint32_t &rank) {
    uint32_t below = 0;
    for (int b0 = 0; b0 < ORDER_BINS; b0 += 16) {
        uint32_t block = 0;
        for (int i = 0; i < 16; ++i) block += hist[b0 + i];
        if (rank - below < block) {
            for (int d = b0; d < b0 + 16; ++d) {
                const uint32_t c = hist[d];
                if (rank - below < c) {
                    prefix |= (uint64_t)d << order64_shift(pass);
                    rank -= below;
                    return true;
                }
                below += c;
            }
        }
        below += block;
    }
    return false;
}

}  // namespace seir

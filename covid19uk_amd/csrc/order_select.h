// One step of an MSB-first radix select: the one definition of "given the histogram of a digit and a rank, which digit
// holds that rank, and which rank is it among the values of that digit", host + device (plain C++ for
// tests/test_forecast_quantiles_host.py and tests/test_rt_quantiles_host.py, __device__ for order_stats_cell of
// order_stats_kernels.h), for keys of 32 and of 64 bits: the functions are templates on the key type K.
//
// int32 values (K = uint32_t): the order is that of signed int32; a value is compared through its key, the value with the
// sign bit flipped, as an unsigned number.
// fp64 values (K = uint64_t): the order is DEFINED as that of IEEE-754 totalOrder on the bit pattern: a value is compared
// through its key,
//   key = bits ^ (bits >> 63 ? ~0ull : 1ull << 63),
// as an unsigned 64-bit number (a negative value has all its bits flipped, a positive one its sign bit).  On arrays without
// NaN this is the order of np.sort, bit for bit, except that -0.0 sorts before +0.0 (np.sort leaves equal values in any
// order); NaNs sort by sign and payload, the negative ones before -inf and the positive ones behind +inf (np.sort puts every
// NaN last).
//
// The key is cut into order_passes<K>() digits of ORDER_DIGIT_BITS bits (ORDER_PASSES == 4, ORDER64_PASSES == 8), the most
// significant first.  A rank's state is (prefix, rank): the digits found so far, a K, and the rank that remains among the
// values whose key starts with them, 32 bits; it starts as (0, r).  Pass p counts, for the values whose key agrees with the
// prefix on the digits above digit p, digit p into a histogram of ORDER_BINS bins; order_select_narrow moves the state one
// digit down.  After the last pass the prefix IS the key of the r-th value in that order (np.sort(values)[r] for int32),
// and order_value gives the value, or the double's bits, back.  Everything is integer arithmetic and exact for any values
// and any n < 2^32.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SEIR_OS_HD __host__ __device__ __forceinline__
#else
#define SEIR_OS_HD inline
#endif

namespace seir {

constexpr int ORDER_DIGIT_BITS = 8;
constexpr int ORDER_BINS = 1 << ORDER_DIGIT_BITS;
constexpr int ORDER_PASSES = 32 / ORDER_DIGIT_BITS;
constexpr int ORDER64_PASSES = 64 / ORDER_DIGIT_BITS;
constexpr int ORDER_MAX_RANKS = 16;    // SEIR_ORDER_STATS_MAX_RANKS

template <typename K>
constexpr int order_passes() { return 8 * (int)sizeof(K) / ORDER_DIGIT_BITS; }

// The two key maps and their inverses (a 64-bit key with its top bit set came from a positive value).
SEIR_OS_HD uint32_t order_key(int32_t v) { return (uint32_t)v ^ 0x80000000u; }
SEIR_OS_HD int32_t order_value(uint32_t key) { return (int32_t)(key ^ 0x80000000u); }
SEIR_OS_HD uint64_t order_key(uint64_t bits) { return bits ^ ((bits >> 63) ? ~0ull : 1ull << 63); }
SEIR_OS_HD uint64_t order_value(uint64_t key) { return key ^ ((key >> 63) ? 1ull << 63 : ~0ull); }

// Bit position of digit `pass` (pass 0 is the most significant).
template <typename K>
SEIR_OS_HD int order_shift(int pass) { return 8 * (int)sizeof(K) - ORDER_DIGIT_BITS * (pass + 1); }
// The digit of `key` that pass `pass` counts.
template <typename K>
SEIR_OS_HD uint32_t order_digit(K key, int pass) { return (uint32_t)(key >> order_shift<K>(pass)) & (uint32_t)(ORDER_BINS - 1); }
// Does `key` agree with `prefix` on every digit above digit `pass`?  (Always in pass 0.)
template <typename K>
SEIR_OS_HD bool order_matches(K key, K prefix, int pass) {
    return pass == 0 || ((key ^ prefix) >> (order_shift<K>(pass) + ORDER_DIGIT_BITS)) == (K)0;
}

// hist [ORDER_BINS]: the counts of digit `pass` among the values that match `prefix`; 0 <= rank < sum(hist).
// Moves (prefix, rank) one digit down: the smallest digit d with hist[0] + .. + hist[d] > rank, and the rank among that
// bin's values.  The bins are summed in blocks of 16 first, so that the loads of a block do not wait for one another.
// Returns false, and leaves the state alone, if rank >= sum(hist): the caller's counts do not add up.
template <typename K>
SEIR_OS_HD bool order_select_narrow(const uint32_t *hist, int pass, K &prefix, uint32_t &rank) {
    uint32_t below = 0;
    for (int b0 = 0; b0 < ORDER_BINS; b0 += 16) {
        uint32_t block = 0;
        for (int i = 0; i < 16; ++i) block += hist[b0 + i];
        if (rank - below < block) {
            for (int d = b0; d < b0 + 16; ++d) {
                const uint32_t c = hist[d];
                if (rank - below < c) {
                    prefix |= (K)d << order_shift<K>(pass);
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

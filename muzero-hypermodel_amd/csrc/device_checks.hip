// device_checks.hip -- the cut-down arithmetic sequences of narrow_device.h against the plain forms they claim to
// reproduce, evaluated side by side on the GPU over whole operand domains (mzmcts_device_numerics, include/mzmcts.h).
//
// A translation unit of its own, compiled with the flags of every other source: "the same bits as expf" is a statement
// about the code the compiler emits for expf under exactly those flags.  Each thread takes one operand, evaluates the
// short form and the plain form, compares the result bits and measures the distance to a float64 evaluation; a launch
// reduces to a mismatch count, a few offending operand patterns and the largest distance.  Nothing per operand leaves
// the device.  Plain C++ throughout: results go out through ordinary atomics on global memory.
//
// Two checks have no short form: logf and powf as trainer_kernels.hip calls them (the soft-max normaliser's logarithm,
// the PER priority's power), measured against float64 over the whole operand domain the loss kernel can present.  The
// exponent of powf reaches the kernel as an argument, as per_alpha does there, so the compiler sees the same general call.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mzmcts.h"
#include "fc_net_device.h"
#include "kernel_common.h"
#include "narrow_device.h"
#include "tree_device.h"

namespace mz {

constexpr int kCheckThreads = 256;
constexpr int kBadSlots = 8;

struct NumericsResult {
    unsigned long long mismatches;
    unsigned long long smallest;         // the smallest offending pattern
    unsigned long long bad[kBadSlots];   // the first offenders, in arrival order
    unsigned long long arrivals;         // offenders that asked for a slot
    unsigned long long worst_bits;       // bit pattern of the largest distance (a non-negative double: ordered like an integer)
};

__device__ __forceinline__ uint32_t f32_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ uint64_t f64_bits(double v) { return __builtin_bit_cast(uint64_t, v); }
__device__ __forceinline__ double f64_from(uint64_t b) { return __builtin_bit_cast(double, b); }

// spacing of float32 numbers at |reference| (the denormal spacing below 2^-126)
__device__ __forceinline__ double f32_ulp_at(double reference) {
    int e = 0;
    (void)frexp(fabs(reference), &e);             // |reference| = m 2^e, 0.5 <= m < 1
    if (reference == 0.0 || e - 1 < -126) e = -125;
    return ldexp(1.0, e - 1 - 23);
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ bool same_f64(double a, double b) { return f64_bits(a) == f64_bits(b) || (a != a && b != b); }

// distance between two doubles of one sign in units of the last place (0 for equal, huge across signs / NaNs)
__device__ __forceinline__ double f64_ulps_apart(double a, double b) {
    if (same_f64(a, b)) return 0.0;
    if (a != a || b != b || ((f64_bits(a) ^ f64_bits(b)) >> 63)) return 0x1p62;
    const uint64_t x = f64_bits(a) & ~(1ull << 63), y = f64_bits(b) & ~(1ull << 63);
    return static_cast<double>(x > y ? x - y : y - x);
}

// ---- operands of the structured fp64 checks ---------------------------------------------------------------------
// Quotients: case i = (denominator 1 + i % 32768) x (sign) x (exponent field) x (mantissa kind: all zeros, all ones, two
// seeded ones that differ from case to case).  `all_exponents`: the exponent field runs over 0 .. 2047 (subnormals,
// infinities and NaNs included) instead of 1023 - 401 .. 1023 + 401.
constexpr uint64_t kQuotientDenominators = 32768;
constexpr uint64_t kQuotientExponents = 803;          // -401 .. 401
constexpr uint64_t kQuotientMantissas = 4;
__host__ __device__ constexpr uint64_t quotient_cases(bool all_exponents) {
    return kQuotientDenominators * 2 * (all_exponents ? 2048 : kQuotientExponents) * kQuotientMantissas;
}
__device__ __forceinline__ void quotient_case(uint64_t i, bool all_exponents, double& n, double& d) {
    d = static_cast<double>(1 + i % kQuotientDenominators);
    uint64_t t = i / kQuotientDenominators;
    const uint64_t sign = t & 1;
    t >>= 1;
    const uint64_t n_exp = all_exponents ? 2048 : kQuotientExponents;
    const uint64_t field = all_exponents ? t % n_exp : 1023 - 401 + t % n_exp;
    const uint64_t kind = t / n_exp;
    const uint64_t mantissa = kind == 0 ? 0ull : kind == 1 ? 0xFFFFFFFFFFFFFull : splitmix64(i) & 0xFFFFFFFFFFFFFull;
    n = f64_from((sign << 63) | (field << 52) | mantissa);
}

// Min-max normalisation: minimum = r + 0.997 q with r, q born float32 (what a backup hands to the statistics), the range
// one of 64 sizes (1, 2, 4 .. 2^15 units of the last place of the minimum; then 48 steps from 1e-13 up to 1e3), the
// value at the minimum, at the maximum, next to either (inside) or at a seeded interior point.
constexpr uint64_t kNormalizedRanges = 64, kNormalizedValues = 8;
__device__ __forceinline__ void normalized_case(uint64_t i, double& minimum, double& maximum, double& v) {
    const uint64_t h = splitmix64(i * 2 + 1), g = splitmix64(i * 2);
    const uint64_t range_kind = i % kNormalizedRanges, value_kind = (i / kNormalizedRanges) % kNormalizedValues;
    // magnitudes from 1e-3 up to ~500, both signs; every fourth case starts at exactly 1.0 (one fp64 ulp at 1.0 upwards)
    const float r = static_cast<float>(static_cast<int>(h & 0xFFFFF) - 0x80000) * (1.0f / 1024.f) *
                    ((h >> 20) & 1 ? 1.0f : 0x1p-9f);
    const float q = static_cast<float>(static_cast<int>((h >> 24) & 0xFFFFF) - 0x80000) * (1.0f / 4096.f);
    minimum = ((i >> 9) & 3) == 0 ? 1.0 : static_cast<double>(r) + 0.997 * static_cast<double>(q);
    if (minimum == 0.0) minimum = 0.25;
    if (range_kind < 16) {
        const uint64_t steps = 1ull << range_kind;
        const uint64_t b = f64_bits(minimum);
        maximum = f64_from(minimum > 0.0 ? b + steps : (b & ~(1ull << 63)) > steps ? b - steps : 0x3FF0000000000000ull);
    } else {
        maximum = minimum + pow(10.0, -13.0 + static_cast<double>(range_kind - 16) * (16.0 / 47.0));
    }
    if (!(maximum > minimum)) maximum = nextafter(minimum, INFINITY);   // (a range below the spacing at the minimum)
    const double span = maximum - minimum;
    const double u = static_cast<double>(g >> 11) * 0x1p-53;
    switch (value_kind) {
        case 0: v = minimum; break;
        case 1: v = maximum; break;
        case 2: v = nextafter(minimum, maximum); break;
        case 3: v = nextafter(maximum, minimum); break;
        default: v = minimum + u * span; break;
    }
    v = fmin(fmax(v, minimum), maximum);
}

// One operand per thread: pattern = first + global id.  `bad` is what the call counts (see include/mzmcts.h per check).
__global__ __launch_bounds__(kCheckThreads) void device_numerics_kernel(int which, unsigned long long first,
                                                                        unsigned long long count, float exponent,
                                                                        NumericsResult* out) {
    const unsigned long long gid = static_cast<unsigned long long>(blockIdx.x) * kCheckThreads + threadIdx.x;
    const bool live = gid < count;
    const unsigned long long pattern = first + (live ? gid : 0ull);
    bool bad = false;
    double distance = 0.0;
    if (which == MZMCTS_NUMERICS_EXP) {
        const float x = __builtin_bit_cast(float, static_cast<uint32_t>(pattern));
        if (x == x) {
            const float fast = exp_nonpositive(x), plain = expf(x);
            bad = f32_bits(fast) != f32_bits(plain);
            const double reference = exp(static_cast<double>(x));
            distance = fabs(static_cast<double>(fast) - reference) / f32_ulp_at(reference);
        }
    } else if (which == MZMCTS_NUMERICS_RECIPROCAL) {
        const float d = __builtin_bit_cast(float, static_cast<uint32_t>(pattern));
        if (d == d) {
            const float fast = reciprocal_of_sum(d), plain = 1.0f / d;
            bad = f32_bits(fast) != f32_bits(plain);
            const double reference = 1.0 / static_cast<double>(d);
            distance = fabs(static_cast<double>(fast) - reference) / f32_ulp_at(reference);
        }
    } else if (which == MZMCTS_NUMERICS_INVERSE_TRANSFORM) {
        const float x = __builtin_bit_cast(float, static_cast<uint32_t>(pattern));
        if (x == x) {
            const float fast = inverse_value_transform_narrow(x, inverse_transform_reciprocal());
            const float plain = inverse_value_transform(x);
            bad = f32_bits(fast) != f32_bits(plain);
            // models.py:656-661 in float64; the distance is absolute, in units of sqrt(|value| + 1)
            const double ax = fabs(static_cast<double>(x));
            const double z = (sqrt(1.0 + 4.0 * 0.001 * (ax + 1.0 + 0.001)) - 1.0) / (2.0 * 0.001);
            const double reference = (x > 0.f ? 1.0 : x < 0.f ? -1.0 : 0.0) * (z * z - 1.0);
            distance = fabs(static_cast<double>(fast) - reference) / sqrt(fabs(reference) + 1.0);
        }
    } else if (which == MZMCTS_NUMERICS_QUOTIENT || which == MZMCTS_NUMERICS_QUOTIENT_GUARDED) {
        const bool guarded = which == MZMCTS_NUMERICS_QUOTIENT_GUARDED;
        double n, d;
        quotient_case(pattern, guarded, n, d);
        const double fast = quotient_with(n, d, refined_reciprocal(d)), plain = n / d;
        const bool differ = !same_f64(fast, plain);
        // (a numerator of -0.0 is outside the domain: the short form answers +0.0, see quotient_with)
        bad = guarded ? differ && !leaves_plain_range(n) && f64_bits(n) != (1ull << 63) : differ;
        if (bad) distance = f64_ulps_apart(fast, plain);
    } else if (which == MZMCTS_NUMERICS_NORMALIZED) {
        MinMax mm;
        double v;
        normalized_case(pattern, mm.minimum, mm.maximum, v);
        const Normalizer fast = make_normalizer(mm, 0ull);
        const double plain = (v - mm.minimum) / (mm.maximum - mm.minimum);
        const double single = normalized_value(fast, v);
        double pair_a, pair_b;
        normalized_pair(fast, v, mm.maximum, pair_a, pair_b);
        const bool in_range = !leaves_plain_range(v) && !leaves_plain_range(mm.minimum) && !leaves_plain_range(mm.maximum);
        bad = !in_range || !fast.fast || !same_f64(single, plain) || !same_f64(pair_a, plain) || !same_f64(pair_b, 1.0);
        if (bad) distance = fmax(f64_ulps_apart(single, plain), f64_ulps_apart(pair_a, plain));
    } else if (which == MZMCTS_NUMERICS_LOG) {   // "offending" = more than 4 float32 ulps from float64 log
        const float x = __builtin_bit_cast(float, static_cast<uint32_t>(pattern));
        const double reference = log(static_cast<double>(x));
        // log(1) = 0 exactly: anything else there is infinitely many ulps away; elsewhere the spacing at the reference
        distance = (reference == 0.0) ? (logf(x) == 0.f ? 0.0 : 0x1p62)
                                      : fabs(static_cast<double>(logf(x)) - reference) / f32_ulp_at(reference);
        bad = distance > 4.0;
    } else if (which == MZMCTS_NUMERICS_POW_HALF || which == MZMCTS_NUMERICS_POW_ONE) {
        const float x = __builtin_bit_cast(float, static_cast<uint32_t>(pattern));
        const double reference = pow(static_cast<double>(x), static_cast<double>(exponent));
        const float got = powf(x, exponent);
        distance = (reference == 0.0) ? (got == 0.f ? 0.0 : 0x1p62)
                                      : fabs(static_cast<double>(got) - reference) / f32_ulp_at(reference);
        bad = distance > 4.0;
    } else {   // MZMCTS_NUMERICS_PLAIN_RANGE: "offending" = the guard fires on the double with this bit pattern
        bad = leaves_plain_range(f64_from(pattern));
    }
    bad = bad && live;
    if (!live) distance = 0.0;
    // the largest distance of the wavefront, then one atomic per wavefront (non-negative doubles order like integers)
    if (!(distance == distance)) distance = 0x1p62;
    for (int m = 1; m < 64; m <<= 1) distance = fmax(distance, __shfl_xor(distance, m, 64));
    if ((threadIdx.x & 63) == 0 && distance > 0.0) atomicMax(&out->worst_bits, static_cast<unsigned long long>(f64_bits(distance)));
    if (bad) {
        atomicAdd(&out->mismatches, 1ull);
        atomicMin(&out->smallest, pattern);
        const unsigned long long slot = atomicAdd(&out->arrivals, 1ull);
        if (slot < kBadSlots) out->bad[slot] = pattern;
    }
}

}  // namespace mz

extern "C" {

#define MZ_CHECK_HIP(call)                               \
    do {                                                 \
        if ((call) != hipSuccess) {                      \
            if (d_out) (void)hipFree(d_out);             \
            return MZMCTS_ERR_HIP;                       \
        }                                                \
    } while (0)

int mzmcts_device_numerics(int32_t which, uint64_t first, uint64_t count, uint64_t* mismatches_out, uint64_t* first_bad_out,
                           double* worst_out) {
    if (!mismatches_out || !first_bad_out || !worst_out) return MZMCTS_ERR_INVALID;
    if (count == 0 || count > MZMCTS_NUMERICS_MAX_COUNT) return MZMCTS_ERR_INVALID;
    uint64_t domain = 0, low = 0;
    switch (which) {
        case MZMCTS_NUMERICS_EXP:
        case MZMCTS_NUMERICS_RECIPROCAL:
        case MZMCTS_NUMERICS_INVERSE_TRANSFORM: domain = 1ull << 32; break;               // float32 bit patterns
        case MZMCTS_NUMERICS_QUOTIENT: domain = mz::quotient_cases(false); break;
        case MZMCTS_NUMERICS_QUOTIENT_GUARDED: domain = mz::quotient_cases(true); break;
        case MZMCTS_NUMERICS_NORMALIZED: domain = 1ull << 40; break;                     // seeded cases: any index below
        case MZMCTS_NUMERICS_PLAIN_RANGE: domain = 0; break;                             // float64 bit patterns: all 2^64
        case MZMCTS_NUMERICS_LOG: low = 0x3F800000ull; domain = 0x44800000ull; break;     // the floats of [1, 1024)
        case MZMCTS_NUMERICS_POW_HALF:
        case MZMCTS_NUMERICS_POW_ONE: domain = 0x7F800000ull; break;                     // +0.0 .. the largest finite float
        default: return MZMCTS_ERR_INVALID;
    }
    if (first < low) return MZMCTS_ERR_INVALID;
    if (domain != 0 && (first >= domain || count > domain - first)) return MZMCTS_ERR_INVALID;
    if (domain == 0 && first + count < first && first + count != 0) return MZMCTS_ERR_INVALID;   // wraps past 2^64

    mz::NumericsResult host{};
    host.smallest = ~0ull;
    mz::NumericsResult* d_out = nullptr;
    MZ_CHECK_HIP(hipMalloc(&d_out, sizeof(host)));
    MZ_CHECK_HIP(hipMemcpy(d_out, &host, sizeof(host), hipMemcpyHostToDevice));
    const unsigned blocks = static_cast<unsigned>((count + mz::kCheckThreads - 1) / mz::kCheckThreads);
    mz::device_numerics_kernel<<<dim3(blocks), dim3(mz::kCheckThreads)>>>(
        which, first, count, which == MZMCTS_NUMERICS_POW_HALF ? 0.5f : 1.0f, d_out);
    MZ_CHECK_HIP(hipGetLastError());
    MZ_CHECK_HIP(hipMemcpy(&host, d_out, sizeof(host), hipMemcpyDeviceToHost));   // (waits for the kernel)
    (void)hipFree(d_out);
    *mismatches_out = host.mismatches;
    // the smallest offender first, then the others in arrival order
    int n_out = 0;
    for (int i = 0; i < mz::kBadSlots; ++i) first_bad_out[i] = 0;
    if (host.mismatches > 0) first_bad_out[n_out++] = host.smallest;
    for (int i = 0; i < mz::kBadSlots && static_cast<uint64_t>(i) < host.mismatches && n_out < mz::kBadSlots; ++i)
        if (host.bad[i] != host.smallest) first_bad_out[n_out++] = host.bad[i];
    *worst_out = __builtin_bit_cast(double, static_cast<uint64_t>(host.worst_bits));
    return MZMCTS_OK;
}

}  // extern "C"

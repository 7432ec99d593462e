// select_action.h -- SelfPlay.select_action (reference self_play.py:223-246) at any temperature, over caller-provided
// MT19937 storage.  One source for the device (select_action_general_kernel and device_select_action_kernel,
// mzmcts_rng.hip) and for plain g++ (tests/select_action_check.cpp runs the very code the kernels run, against
// HostStream::select_action on the machine's libm).
//
// For a finite T > 0 the reference computes
//     w = visit_counts ** (1 / T);  p = w / sum(w);  numpy.random.choice(actions, p=p)
// i.e. libm's pow per child (glibc's, restated in glibc_libm.h), Python's left-to-right sum, one division per child,
// then RandomState.choice: the running sum of p divided by its last value, one legacy double (two 32-bit words), right
// bisect.  Every addition and division below is in that order; the library is built with -ffp-contract=off.
//
// The whole-move kernels sample T = 0, +inf and 1 / k (k = 1..4) in their epilogues (kernel_common.h
// device_select_action); what that function answers -2 for comes here.
#pragma once
#include "np_legacy_rng.h"

namespace mz {

// visits ** inv_temperature as libm's pow returns it; inv_temperature = 1 / T > 0, computed once per row in fp64.
// glibc_pow covers exponents from 2^-65 up; below that libm answers pow(0, y) = 0, pow(1, y) = 1 and 1 + y (= 1) for
// x > 1 without going through its log / exp kernels.
MZ_HD inline double visit_weight(int32_t visits, double inv_temperature) {
    if (inv_temperature < 0x1p-65) return visits == 0 ? 0.0 : (visits == 1 ? 1.0 : 1.0 + inv_temperature);
    return libm::glibc_pow(static_cast<double>(visits), inv_temperature);
}

// numpy.random.choice(n, p = w / sum(w)) on the stream (key, pos): `words` grows by the two words of the legacy double.
template <typename WeightOf>
MZ_HD inline int choice_by_weight(WeightOf weight, int n, uint32_t* key, int32_t* pos, uint32_t* words) {
    double total = 0.0;
    for (int i = 0; i < n; ++i) total = total + weight(i);
    double total_p = 0.0;
    for (int i = 0; i < n; ++i) total_p += weight(i) / total;
    const int32_t a = static_cast<int32_t>(mt_next(key, pos) >> 5);
    const int32_t b = static_cast<int32_t>(mt_next(key, pos) >> 6);
    *words += 2u;
    const double u = (a * 67108864.0 + b) / 9007199254740992.0;
    double run = 0.0;
    int idx = 0;
    for (; idx < n; ++idx) {
        run += weight(idx) / total;
        if (!(run / total_p <= u)) break;
    }
    return idx;
}

// Does temperature T take the pow path for a row whose visit counts sum to `simulations`?  Not T = 0, not +inf, and
// not 1 / k while simulations ** k is an integer a double holds exactly (the bound the move batches check: 9e15).
MZ_HD inline bool general_temperature(double temperature, double simulations) {
    if (temperature == 0.0 || !(temperature < INFINITY)) return false;
    const int k = exact_inverse_temperature(temperature);
    if (k == 0) return true;
    double power = simulations;
    for (int r = 1; r < k; ++r) power = power * simulations;
    return !(power < 9.0e15);
}

// Can a row of n children whose visit counts sum to `simulations` be sampled at T?  T = 0 and +inf always; otherwise T
// must be finite and positive with n * simulations ** (1 / T) finite, so that no weight, and no sum of weights,
// overflows (the reference would fail inside numpy.random.choice on NaN probabilities).
MZ_HD inline bool temperature_samplable(double temperature, int n, double simulations) {
    if (temperature == 0.0 || temperature == INFINITY) return true;
    if (!(temperature > 0.0)) return false;              // negative, NaN
    const double inv = 1.0 / temperature;
    if (!(inv < 0x1p62)) return false;                   // (glibc_pow's exponent range; such a power overflows anyway)
    const double top = simulations < 1.0 ? 1.0 : simulations;
    const double bound = static_cast<double>(n) * visit_weight(top > 2147483647.0 ? 2147483647 : static_cast<int32_t>(top), inv);
    return bound < INFINITY;
}

// SelfPlay.select_action at any temperature that temperature_samplable admits -> chosen child slot.
// `weights`: scratch of n doubles (each pow is computed once), untouched on the T = 0 / +inf / exact 1 / k paths, which
// are device_select_action's.
template <typename VisitOf>
MZ_HD inline int select_action_any(VisitOf visit_of, int n, double temperature, double* weights, uint32_t* key,
                                   int32_t* pos, uint32_t* words) {
    if (temperature == 0.0) {
        int best = 0, best_v = visit_of(0);
        for (int i = 1; i < n; ++i) {
            const int v = visit_of(i);
            if (v > best_v) {
                best_v = v;
                best = i;
            }
        }
        return best;
    }
    if (temperature == INFINITY) return static_cast<int>(mt_below(key, pos, static_cast<uint32_t>(n), words));
    double simulations = 0.0;
    for (int i = 0; i < n; ++i) simulations += static_cast<double>(visit_of(i));
    if (!general_temperature(temperature, simulations)) {
        const int k = exact_inverse_temperature(temperature);
        return choice_by_weight(
            [&](int i) {
                const double v = static_cast<double>(visit_of(i));
                double w = v;
                for (int r = 1; r < k; ++r) w = w * v;
                return w;
            },
            n, key, pos, words);
    }
    const double inv = 1.0 / temperature;
    for (int i = 0; i < n; ++i) weights[i] = visit_weight(visit_of(i), inv);
    return choice_by_weight([&](int i) { return weights[i]; }, n, key, pos, words);
}

}  // namespace mz

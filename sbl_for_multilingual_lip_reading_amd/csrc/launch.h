// Host helpers shared by the launchers (included by sbl_common.h): compile-time dispatch on the matrix-product precision and
// the once-per-device raise of a kernel's dynamic-LDS cap.
#pragma once
#include <type_traits>

#include "tuning.h"

template <int V>
using sbl_int = std::integral_constant<int, V>;

// Calls f(sbl_int<P>{}) for the current matrix-product precision P (g_sbl_prec: 6 / 3 / 1 bf16 MFMA terms, else 0 = fp32) and
// returns what f returns.  Launchers of bf16-only kernels have ruled out P == 0 before they get here; they answer
// `if constexpr (P == 0)` with "not taken", so that no fp32 instantiation of such a kernel exists.
template <class F>
static inline auto sbl_with_prec(F&& f) {
    switch (g_sbl_prec) {
        case 6: return f(sbl_int<6>{});
        case 3: return f(sbl_int<3>{});
        case 1: return f(sbl_int<1>{});
        default: return f(sbl_int<0>{});
    }
}
// Same for kernels with a wave-group K split (template argument NH, 256 * NH threads): f(sbl_int<P>{}, sbl_int<NH>{}) with
// NH = 2 when the caller asks for it (nh == 2) and the precision is a split-bf16 one; the fp32 body always runs NH = 1.
template <class F>
static inline auto sbl_with_prec_nh(int nh, F&& f) {
    return sbl_with_prec([&](auto p) {
        if constexpr (decltype(p)::value != 0)
            if (nh == 2) return f(p, sbl_int<2>{});
        return f(p, sbl_int<1>{});
    });
}

// Kernels that take more than 64 KB of dynamic LDS: raise the cap of kernel `fn` to `bytes`, once per device.  `flags` is
// that kernel instantiation's own array (a function-local static of a named function or function template, never of a
// generic lambda).  The caller decides what a failure means (fall through to the next route, or SBL_HIP).
static inline hipError_t sbl_raise_lds_cap(const void* fn, int bytes, bool (&flags)[64]) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (!flags[dev & 63]) {
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return e;
        flags[dev & 63] = true;
    }
    return hipSuccess;
}

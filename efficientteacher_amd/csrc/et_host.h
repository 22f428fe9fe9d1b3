// Host-only helpers shared by the launch sites of every kernel file: the run-time codes of the C ABI (dtype, activation) become
// compile-time arguments ONCE, so that a launch and its argument list are written once per entry point.
#pragma once
#include <type_traits>
#include "et_device.h"
#include "../../include/et_hip.h"

enum { ACT_NONE = 0, ACT_SILU = 1, ACT_RELU = 2 };

// f(TypeTag<T>) for the storage type of an ET_* dtype; -2 for any other value (the launch functions: all three types)
template <typename T> struct TypeTag { using type = T; };
template <typename F> static int with_dtype(int dtype, F&& f) {
    if (dtype == ET_F32) return f(TypeTag<float>{});
    if (dtype == ET_BF16) return f(TypeTag<uint16_t>{});
    if (dtype == ET_F16) return f(TypeTag<et_f16>{});
    return -2;
}
// f(std::integral_constant<int, ACT_*>) for an activation code; any other value is ACT_NONE
template <typename F> static auto with_act(int act, F&& f) {
    if (act == ACT_SILU) return f(std::integral_constant<int, ACT_SILU>{});
    if (act == ACT_RELU) return f(std::integral_constant<int, ACT_RELU>{});
    return f(std::integral_constant<int, ACT_NONE>{});
}

// The kernels that move 16 bytes per lane: elements per vector for a dtype code (every code but ET_F32 counts as 16-bit here; the
// dispatch rejects the unknown ones), and "each of these channel counts / pixel strides is a whole number of vectors".
static int et_vec(int dtype) { return dtype == ET_F32 ? 4 : 8; }
template <typename... N> static bool et_whole_vecs(int vec, N... n) { return (... && (n % vec == 0)); }

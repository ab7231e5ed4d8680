// Shape dispatch of the one-pass attention units (csrc/attention_qkv*.hip): a run-time count of 32-element pieces becomes
// the compile-time unroll class of a kernel.  Private to those units.
#pragma once

#include <stdint.h>

#include <type_traits>

namespace {

template <int N>
using Int = std::integral_constant<int, N>;

// f(Int<P>{}): P is the smallest of 1, 2, 4, ... MAX with n <= P, and MAX for every n beyond it (MAX = 8 or 16)
template <int MAX, typename F>
void withPieces(uint32_t n, F&& f) {
    static_assert(MAX == 8 || MAX == 16, "the classes end at 8 or 16 pieces");
    if (n <= 1u) f(Int<1>{});
    else if (n <= 2u) f(Int<2>{});
    else if (n <= 4u) f(Int<4>{});
    else if (MAX == 8 || n <= 8u) f(Int<8>{});
    else if constexpr (MAX == 16) f(Int<16>{});
}

}  // namespace

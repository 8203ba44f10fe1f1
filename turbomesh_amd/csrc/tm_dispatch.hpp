// A run-time integer as a template argument: dispatch_int<LO, HI>(value, f) calls f(std::integral_constant<int, N>{}) for the N in
// LO .. HI that equals `value`.  A value outside the range is taken as HI; a caller for which that is an error checks the range first.
#pragma once
#include <type_traits>

namespace tmh {

template <int LO, int HI, class F>
inline auto dispatch_int(int value, F&& f) -> decltype(f(std::integral_constant<int, HI>{})) {
    if constexpr (LO < HI) {
        if (value != LO) return dispatch_int<LO + 1, HI>(value, f);
    }
    return f(std::integral_constant<int, LO>{});
}

}  // namespace tmh

// Run-time int -> template argument, the one way the launch wrappers do it. Plain C++17 (no torch /
// HIP headers): also compiled into tests/native/host_plan_test.cpp.
#pragma once
#include <type_traits>

namespace penroz {

template <int... Vs>
struct IntList {};

// f(integral_constant<int, V>...) for the Vs equal to the run-time values, one (list, value) pair
// per template argument of the kernel; false (f not called) when some value is in no list.
template <class F>
bool dispatch_exact(F&& f) {
  f();
  return true;
}
template <class F, int... Vs, class... Rest>
bool dispatch_exact(F&& f, IntList<Vs...>, int v, Rest... rest) {
  return ((v == Vs && dispatch_exact([&](auto... t) { f(std::integral_constant<int, Vs>{}, t...); }, rest...)) || ...);
}

// f(integral_constant<int, V>) for the first V >= v of an ascending list; false when v is above all.
template <class F, int... Vs>
bool dispatch_bucket(F&& f, IntList<Vs...>, int v) {
  return ((v <= Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

}  // namespace penroz

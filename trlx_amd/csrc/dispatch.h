// Runtime value -> compile-time constant, for the host side of every kernel
// file.  Host only, no ATen, nothing kernel-specific: attn_host.h builds its
// head-dim and flash-mode tables on top of this, norms.hip uses it as it is.
#pragma once

#include <type_traits>

// f(std::true_type{}) or f(std::false_type{}): inside a generic lambda the
// argument's ::value is a constant expression, usable as a template argument.
template <typename F>
void dispatch_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

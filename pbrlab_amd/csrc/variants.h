// variants.h -- how a launcher turns a runtime property of the scene into a template argument of its kernel.  Host side only: every
// launcher (kernels.hip, features.hip, emission.hip, rays.hip, temporal.hip, query.hip) selects its instance through these.
#pragma once

#include <type_traits>

#include "dscene.h"
#include "knobs.h"

namespace pb {

// the Q tree serves the scenes whose tree was built on the host (PBRHIP_WIDE=0: never)
static inline bool use_wide(const DScene& sc, const Knobs& k) { return sc.wide != nullptr && k.wide; }
// A runtime property of the scene becomes a template argument here and nowhere else: with_flags(f, a, b, ...) calls the generic lambda f
// with one std::bool_constant per flag, which the lambda's launch names as a template argument (k_trace<st, c, w, first>).  Every
// combination of the flags is an instance in the code object: a kernel that exists for fewer has a selector of its own.
template <class F>
static inline void with_flags(F&& f) { f(); }
template <class F, class... Bools>
static inline void with_flags(F&& f, bool flag, Bools... rest) {
  if (flag) with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
// the <CURVES, WIDE> of the hooks and of every one-ray-per-lane kernel (k_features, k_motion, ...): the tree the render of this scene
// walks, but the binary tree's instance always carries the curve code
template <class F>
static inline void with_hook_tree(F&& f, const DScene& sc, const Knobs& k) {
  if (use_wide(sc, k)) with_flags([&](auto c) { f(c, std::true_type{}); }, sc.num_curves != 0);
  else f(std::true_type{}, std::false_type{});
}

}  // namespace pb

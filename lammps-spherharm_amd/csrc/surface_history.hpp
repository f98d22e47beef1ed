// surface_history.hpp — the two host-side rules that tie the tangential-spring history of a surface family (SPEC §2.15,
// §2.19) to its live words, on plain host arrays: no HIP, so a stand-alone program can call them.  xi is [n][nsurf][W],
// live is [n] words of one bit per surface; <unsigned, 3> for walls, <unsigned char, 2> for cylinders.
#pragma once
#include <cmath>
#include <cstddef>

namespace shp {

// surface s of particle i is live iff one of its W entries is not 0; false at the first entry that is not finite
template <typename Word, int W>
inline bool history_live_words(const double* xi, size_t n, size_t nsurf, Word* live, size_t* bad_i, size_t* bad_s)
{
  for (size_t i = 0; i < n; ++i) {
    live[i] = 0;
    for (size_t s = 0; s < nsurf; ++s)
      for (int k = 0; k < W; ++k) {
        const double v = xi[(i * nsurf + s) * W + k];
        if (!std::isfinite(v)) {
          *bad_i = i;
          *bad_s = s;
          return false;
        }
        if (v != 0.0) live[i] = (Word)(live[i] | ((Word)1 << s));
      }
  }
  return true;
}

// xi as the boundary hands it out: 0 where the bit is dead (the device never zeroes a dead entry)
template <typename Word, int W>
inline void history_mask_dead(const double* xi, const Word* live, size_t n, size_t nsurf, double* out)
{
  for (size_t i = 0; i < n; ++i)
    for (size_t s = 0; s < nsurf; ++s)
      for (int k = 0; k < W; ++k) out[(i * nsurf + s) * W + k] = ((live[i] >> s) & 1u) ? xi[(i * nsurf + s) * W + k] : 0.0;
}

}  // namespace shp

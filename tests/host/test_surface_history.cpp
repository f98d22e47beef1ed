// Stand-alone host program for csrc/surface_history.hpp: the two pure rules that tie the tangential-spring history of
// a surface family to its live words, for both instantiations (<unsigned, 3>: planar walls, <unsigned char, 2>:
// cylinders).  No HIP.  Prints "ok" and returns 0, or the first failed check and 1.  tests/test_surface_history.py builds
// it plainly and with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "surface_history.hpp"

using namespace shp;

static int fails = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++fails;                                                   \
    }                                                            \
  } while (0)

template <typename Word, int W>
static void run(size_t n, size_t ns)
{
  const size_t top = ns - 1;
  // a non-zero component in any one of the W slots sets exactly that surface's bit of that particle
  for (size_t i = 0; i < n; ++i)
    for (size_t s = 0; s < ns; ++s)
      for (int k = 0; k < W; ++k) {
        std::vector<double> xi(n * ns * W, 0.0);
        xi[(i * ns + s) * W + k] = k % 2 ? -0.25 : 1.5;
        std::vector<Word> live(n, (Word)~(Word)0);   // (stale words: the function owns every one of them)
        size_t bi = 99, bs = 99;
        CHECK((history_live_words<Word, W>(xi.data(), n, ns, live.data(), &bi, &bs)));
        for (size_t j = 0; j < n; ++j) CHECK(live[j] == (j == i ? (Word)((Word)1 << s) : (Word)0));
      }
  // the last surface lands in the word's top bit when the word is full
  if (ns == 8 * sizeof(Word)) {
    std::vector<double> xi(n * ns * W, 0.0);
    xi[((n - 1) * ns + top) * W + (W - 1)] = 3.0;
    std::vector<Word> live(n);
    size_t bi, bs;
    CHECK((history_live_words<Word, W>(xi.data(), n, ns, live.data(), &bi, &bs)));
    CHECK(live[n - 1] == (Word)((Word)1 << (8 * sizeof(Word) - 1)));
    CHECK((Word)(live[n - 1] << 1) == 0);
  }
  // all zero: nothing live; all non-zero: every bit of the ns
  {
    std::vector<double> xi(n * ns * W, 0.0);
    std::vector<Word> live(n, 1);
    size_t bi, bs;
    CHECK((history_live_words<Word, W>(xi.data(), n, ns, live.data(), &bi, &bs)));
    for (size_t j = 0; j < n; ++j) CHECK(live[j] == 0);
    for (double& v : xi) v = -2.0;
    CHECK((history_live_words<Word, W>(xi.data(), n, ns, live.data(), &bi, &bs)));
    const Word full = ns == 8 * sizeof(Word) ? (Word)~(Word)0 : (Word)(((Word)1 << ns) - 1);
    for (size_t j = 0; j < n; ++j) CHECK(live[j] == full);
  }
  // a non-finite entry is reported with its particle and surface
  const double bad[3] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(),
                         -std::numeric_limits<double>::infinity()};
  for (int b = 0; b < 3; ++b)
    for (int k = 0; k < W; ++k) {
      const size_t i = n - 1, s = (top + (size_t)b) % ns;
      std::vector<double> xi(n * ns * W, 0.5);
      xi[(i * ns + s) * W + k] = bad[b];
      std::vector<Word> live(n);
      size_t bi = 99, bs = 99;
      CHECK(!(history_live_words<Word, W>(xi.data(), n, ns, live.data(), &bi, &bs)));
      CHECK(bi == i && bs == s);
    }
  // a dead bit yields zeros in the copy, a live one the device's entries, whatever a dead entry holds
  {
    std::vector<double> xi(n * ns * W), out(n * ns * W, -7.0);
    for (size_t k = 0; k < xi.size(); ++k) xi[k] = 1.0 + (double)k;
    xi[0] = std::numeric_limits<double>::quiet_NaN();   // never zeroed on the device: a dead entry may hold anything
    std::vector<Word> live(n, 0);
    live[n - 1] = (Word)((Word)1 << top);
    if (ns > 1) live[0] = (Word)((Word)1 << 1);
    history_mask_dead<Word, W>(xi.data(), live.data(), n, ns, out.data());
    for (size_t i = 0; i < n; ++i)
      for (size_t s = 0; s < ns; ++s)
        for (int k = 0; k < W; ++k) {
          const size_t at = (i * ns + s) * W + k;
          const bool lv = (i == n - 1 && s == top) || (ns > 1 && i == 0 && s == 1);
          CHECK(lv ? out[at] == xi[at] : (out[at] == 0.0 && !std::signbit(out[at])));
        }
    // the two rules undo each other on an array without zeros among the live entries
    std::vector<Word> back(n);
    size_t bi, bs;
    CHECK((history_live_words<Word, W>(out.data(), n, ns, back.data(), &bi, &bs)));
    for (size_t j = 0; j < n; ++j) CHECK(back[j] == live[j]);
  }
}

int main()
{
  for (size_t ns : {(size_t)2, (size_t)8, (size_t)32}) run<unsigned, 3>(3, ns);
  for (size_t ns : {(size_t)2, (size_t)8}) run<unsigned char, 2>(3, ns);
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}

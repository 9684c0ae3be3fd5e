// env_tables.h -- host tables of the lat-long environment light.  Pure host code: scripts/fuzz/env_check.cpp
// compiles env_tables.cpp alone and checks what it returns.
#pragma once

#include <stdint.h>

#include <vector>

namespace pb {

struct EnvTables {
  bool present = false;        // false: every texel is black -- the scene has no environment
  uint32_t width = 0, height = 0;
  std::vector<float> texels;   // 4 floats per texel: radiance rgb x scale, pdf_env (per steradian) of a direction in the texel
  std::vector<double> weight;  // lum * solid angle per texel (what the texel is picked in proportion to)
  std::vector<float> prob;     // alias table (Vose): texel i is kept with probability prob[i], else alias[i] is taken
  std::vector<uint32_t> alias;
  std::vector<uint32_t> keep;  // prob as the device compares it: texel i is kept when a 32-bit random word is below keep[i]
                               // (ceil(prob 2^32), at most 2^32 - 1: within 2^-32 of prob)
  double norm = 0.0;           // sum of lum * solid angle: pdf_env = lum / norm
};

// luminance the environment is importance-sampled by (Rec. 709 weights: zero exactly for a black texel)
inline double env_lum(double r, double g, double b) { return 0.2126 * r + 0.7152 * g + 0.0722 * b; }
// solid angle of a texel in row `row` of an image `h` rows high and `w` columns wide: (2 pi / w)(cos theta0 - cos theta1)
double env_texel_solid_angle(uint32_t row, uint32_t w, uint32_t h);

// rgb: width x height x 3 floats, row 0 = the top.  Returns 0, or -1 for zero sizes, too many texels or a texel that is negative,
// NaN or infinite (tables are left empty then).  Computed in double precision, stored as float.
int build_env_tables(const float* rgb, uint32_t width, uint32_t height, float scale, EnvTables* out);

}  // namespace pb

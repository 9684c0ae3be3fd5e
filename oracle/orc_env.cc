// orc_env.cc -- the oracle's link to the library's host-only environment tables (pbrlab_amd/csrc/env_tables.cpp).
// The alias table is not restated: the oracle samples from the very tables the library uploads (scripts/fuzz/env_check.cpp checks
// them independently), the way both share include/pbr_glibcf.h.
#include <stdlib.h>
#include <string.h>

#include "../pbrlab_amd/csrc/env_tables.h"

// rgb: h x w x 3, row 0 = the top.  Returns -1 for input build_env_tables rejects, 0 for an all-black map (nothing allocated), 1 with
// *texels (4 floats per texel: rgb x scale, pdf_env), *keep and *alias (one word per texel) allocated with malloc.
extern "C" int orc_env_tables(const float* rgb, uint32_t w, uint32_t h, float scale, float** texels, uint32_t** keep, uint32_t** alias) {
  pb::EnvTables t;
  if (pb::build_env_tables(rgb, w, h, scale, &t)) return -1;
  if (!t.present) return 0;
  const size_t n = (size_t)w * h;
  *texels = (float*)malloc(sizeof(float) * 4 * n);
  *keep = (uint32_t*)malloc(sizeof(uint32_t) * n);
  *alias = (uint32_t*)malloc(sizeof(uint32_t) * n);
  if (!*texels || !*keep || !*alias) {
    free(*texels), free(*keep), free(*alias);
    *texels = nullptr, *keep = *alias = nullptr;
    return -1;
  }
  memcpy(*texels, t.texels.data(), sizeof(float) * 4 * n);
  memcpy(*keep, t.keep.data(), sizeof(uint32_t) * n);
  memcpy(*alias, t.alias.data(), sizeof(uint32_t) * n);
  return 1;
}

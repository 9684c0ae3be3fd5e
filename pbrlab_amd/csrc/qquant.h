// qquant.h -- the quantiser of a Q node (dscene.h::QNode), shared by the host collapse (bvh_build.cpp::build_qtree) and the collapse
// on the device (qtree_gpu.hip): one definition, host and device, so that both builders round a child's box the same way.
#pragma once
#include <math.h>

#include "dscene.h"

namespace pb {

struct QBox {
  float lo[3], hi[3];
};

// Quantises the boxes of up to four children into a QNode (dscene.h).  Per axis: step s = extent / 253, org = the node's
// lower bound; a child's bounds are rounded outwards on that grid and
// then checked -- and moved out further if need be -- with the expression the traversal evaluates, fmaf(q, s, org) in single
// precision; when the grid is too fine for that arithmetic (a step below the resolution of org) the step grows: x 1.03125 eight
// times, then it doubles.  The child references nd->c are left zero.  (min / max are spelled as std::min / std::max evaluate them;
// floor / ceil run in double: IEEE on the device too.)
PB_HD bool quantise_node(const QBox* c, int n, QNode* nd) {
  const float inf = __builtin_huge_valf();
  nd->org[0] = nd->org[1] = nd->org[2] = 0.f, nd->sx = nd->sy = nd->sz = 0.f;
  nd->qlo_x = nd->qlo_y = nd->qlo_z = nd->qhi_x = nd->qhi_y = nd->qhi_z = 0u;
  nd->c[0] = nd->c[1] = nd->c[2] = nd->c[3] = 0u;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    float lo = inf, hi = -inf;
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (i < n) lo = c[i].lo[a] < lo ? c[i].lo[a] : lo, hi = hi < c[i].hi[a] ? c[i].hi[a] : hi;
    if (!(lo <= hi) || !(fabsf(lo) < inf) || !(fabsf(hi) < inf)) return false;
    // (the step need not be a power of two: fmaf(q, s, org) rounds once whatever s is, and the result is checked below)
    float sc = nextafterf((hi - lo) / 253.0f, inf);
    sc = sc < 1.1754944e-38f ? 1.1754944e-38f : sc;
    uint32_t wl = 0, wh = 0;
    for (int tries = 0;; tries++) {
      if (tries > 40 || !(fabsf(sc) < inf)) return false;
      const float org = lo;
      bool ok = true;
      wl = 0, wh = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        if (!ok) continue;
        if (i >= n) {  // unused child (reference kEmptyChild): never visited, any bytes will do
          wl |= 255u << (8 * i);
          continue;
        }
        int ql = (int)floor(((double)c[i].lo[a] - (double)org) / (double)sc);
        int qh = (int)ceil(((double)c[i].hi[a] - (double)org) / (double)sc);
        ql = ql > 255 ? 255 : ql, ql = ql < 0 ? 0 : ql, qh = qh > 255 ? 255 : qh, qh = qh < 0 ? 0 : qh;
        while (ql > 0 && !(fmaf((float)ql, sc, org) <= c[i].lo[a])) ql--;
        while (qh < 255 && !(fmaf((float)qh, sc, org) >= c[i].hi[a])) qh++;
        if (!(fmaf((float)ql, sc, org) <= c[i].lo[a] && fmaf((float)qh, sc, org) >= c[i].hi[a])) ok = false;
        wl |= (uint32_t)ql << (8 * i), wh |= (uint32_t)qh << (8 * i);
      }
      if (ok) {
        nd->org[a] = org;
        if (a == 0) nd->sx = sc, nd->qlo_x = wl, nd->qhi_x = wh;
        else if (a == 1) nd->sy = sc, nd->qlo_y = wl, nd->qhi_y = wh;
        else nd->sz = sc, nd->qlo_z = wl, nd->qhi_z = wh;
        break;
      }
      sc *= tries < 8 ? 1.03125f : 2.0f;
    }
  }
  return true;
}

}  // namespace pb

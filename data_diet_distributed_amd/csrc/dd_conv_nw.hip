// conv3x3_kernel instantiations of the tiles other than the 32x32 narrow one: the 16x16, 8x8
// and 4x4 tiles for channel counts the r2 tiles do not take (narrow, and the wide one at 4x4);
// the kernel template lives in dd_conv_kern.h.
#include "dd_conv_kern.h"

namespace dd {
namespace conv {

int dispatch_small(int w, int k, const Args& a, hipStream_t st) {
  if (w == 16) {
    if (k == 8000 + 100 + 10 + 2) return launch<kNarrow, 16, 8, 1, 1, 2>(a, st);
  } else if (w == 8) {
    if (k == 8000 + 200 + 10 + 2) return launch<kNarrow, 8, 8, 2, 1, 2>(a, st);
    if (k == 8000 + 100 + 10 + 2) return launch<kNarrow, 8, 8, 1, 1, 2>(a, st);
  } else if (w == 4) {
    if (k == 4000 + 1600 + 20 + 1) return launch<kNarrow, 4, 4, 16, 2, 1>(a, st);
    if (k == 4000 + 400 + 10 + 2) return launch<kNarrow, 4, 4, 4, 1, 2>(a, st);
  }
  set_error("dd_conv3x3_forward: no kernel for tile key %d at w=%d", k, w);
  return DD_EINVAL;
}

}  // namespace conv
}  // namespace dd

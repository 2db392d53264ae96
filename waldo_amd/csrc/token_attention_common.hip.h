// What the token attention's forward (token_attention.hip) and backward (token_attention_bwd.hip) share: the tiles,
// the LDS row padding, the 16-byte register type and the host's argument checks of the five operand views.
#pragma once
#include "waldo_common.hip.h"

namespace waldo {

constexpr int kTaQ = 64;    // query rows per workgroup (16 per wavefront)
constexpr int kTaK = 64;    // keys per tile
constexpr int kTaPad = 4;   // floats added to an LDS row

typedef float ta_f32x4 __attribute__((ext_vector_type(4)));

inline bool ta_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The refusals every entry point of the section shares, in the forward's order and words, up to the strides; `blocks`
// is the larger of the row blocks per (b, h) that the entry point's launches make.  WALDO_OK: go on.
inline int ta_check_shape(const char* fn, const int64_t strides[10], float scale, int64_t B, int H, int D, int Nq,
                          int Nk1, int Nk2, int64_t blocks) {
  if (B < 0 || H < 1 || Nq < 0 || Nk1 < 1 || Nk2 < 0) {
    set_error("%s: bad shape B=%lld H=%d Nq=%d Nk1=%d Nk2=%d (B, Nq, Nk2 >= 0; H, Nk1 >= 1)", fn, (long long)B, H, Nq,
              Nk1, Nk2);
    return WALDO_EINVAL;
  }
  if (D != 16 && D != 32 && D != 64) {
    set_error("%s: bad head dimension D=%d (16, 32 or 64)", fn, D);
    return WALDO_EINVAL;
  }
  if (!(scale == scale) || scale == INFINITY || scale == -INFINITY) {
    set_error("%s: bad scale %g (finite)", fn, (double)scale);
    return WALDO_EINVAL;
  }
  if ((int64_t)Nk1 + Nk2 > INT32_MAX - kTaK || B * H > INT32_MAX || B * H * blocks > INT32_MAX) {
    set_error("%s: too large: B=%lld H=%d Nq=%d Nk1=%d Nk2=%d (Nk1 + Nk2 and the %d-row query blocks of all (b, h) stay "
              "below 2^31)", fn, (long long)B, H, Nq, Nk1, Nk2, kTaQ);
    return WALDO_EINVAL;
  }
  const int nstr = Nk2 > 0 ? 10 : 6;
  for (int i = 0; i < nstr; ++i)
    if (strides[i] < 0) {
      set_error("%s: negative stride", fn);
      return WALDO_EINVAL;
    }
  // a (token, head) row is D consecutive floats read in 16-byte pieces.  A token stride that is no whole number of
  // pieces is what a view with a non-unit inner stride (or rows off the 16-byte boundaries) would need: it has no
  // description here.  A batch stride only has to keep the rows of the next sequence on those boundaries.
  for (int i = 0; i < nstr; ++i)
    if (strides[i] % 4 != 0) {
      if (i & 1)
        set_error("%s: bad token stride %lld: rows are D consecutive floats a multiple of 4 floats apart (a view with a "
                  "non-unit inner stride is not served)", fn, (long long)strides[i]);
      else
        set_error("%s: bad batch stride %lld: a multiple of 4 floats (rows on 16-byte boundaries)", fn,
                  (long long)strides[i]);
      return WALDO_EINVAL;
    }
  return WALDO_OK;
}

}  // namespace waldo

// namespace gpu: a tensor seen as [rows, W] through a leading dimension, for the row kernels that take one (kf_glu_*, kf_softmax_*).
#pragma once

#include <cstdint>

#include "tensor.h"

namespace gpu {

// [rows, W] through a leading dimension: a unit stride along the last dim and one uniform row stride over the flattened leading dims
struct RowView {
    Tensor t;          // keeps the storage alive
    int64_t rows, ld;
};
inline bool row_strided(const Tensor &t, int64_t W, int64_t &ld) {
    const int n = t.dim();
    if (n == 0 || (t.shape(n - 1) > 1 && t.stride(n - 1) != 1)) return false;
    ld = -1;
    int64_t inner = 1;   // rows spanned by the dims to the right of d
    for (int d = n - 2; d >= 0; --d) {
        if (t.shape(d) == 1) continue;
        if (ld < 0) ld = t.stride(d);
        else if (t.stride(d) != ld * inner) return false;
        inner *= t.shape(d);
    }
    if (ld < 0) ld = W;   // one row
    return ld >= W;
}
// t itself when one leading dimension describes it (no copy), else its dense copy
inline RowView rows_of(const Tensor &t) {
    const int64_t W = t.shape(-1);
    int64_t ld = 0;
    if (row_strided(t, W, ld)) return {t, W ? t.numel() / W : 0, ld};
    Tensor d = t.dense();
    return {d, W ? d.numel() / W : 0, W};
}

} // namespace gpu

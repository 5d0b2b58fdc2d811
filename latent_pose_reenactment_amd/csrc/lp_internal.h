// internal helpers shared by the translation units of liblp_hip.so (not part of the C ABI)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
int lp_set_error(int code, const char* msg);
int lp_check_launch(const char* what);

// conv_thin.hip: fixed-order reduction of the per-workgroup slabs of wgrad_rows_kernel (thin_rows.h), part[G][T][slabC][wideC] (thin channels
// < thinC live) -> dw[Cout][Cin][T], and of the bias partials bpart[G][wideC] -> dbias (either NULL: none).  thin_x: the thin side is the input.
int lp_wgrad_rows_reduce(const float* part, const float* bpart, float* dw, float* dbias, int G, int T, int slabC, int thinC, int wideC, bool thin_x,
                         hipStream_t stream);

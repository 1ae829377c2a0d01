// The co-resident instances of k_conv_hx (conv_hx_kernel.h, "CO") and their launcher: a translation unit of their own, compiled beside conv_hx.hip.
#include "conv_hx_kernel.h"

#define HX_CO(T_, EP_, IO_) hipLaunchKernelGGL((k_conv_hx<T_, 2, 16, 16, 128, 4, 1, 1, EP_, IO_>), grid, dim3(256), 0, st, a, tx, ty)
#define HX_CO_IO(T_, EP_) do { if (io == 0) HX_CO(T_, EP_, 0); else if (io == 1) HX_CO(T_, EP_, 1); else if (io == 2) HX_CO(T_, EP_, 2); else HX_CO(T_, EP_, 3); } while (0)

// the launch conv_hx_try would put on the 8-wave 16 x 16 x 128 tile, on the co-resident instance (same grid, same arguments).  ep: the epilogue family conv_hx_try chose (0 plain,
// 1 pooled, 2 masked); io: bit 0 pre-split input, bit 1 S16 output.  1 = launched, -1 = no such instance.
int conv_hx_co_launch(const ConvArgs& a, dim3 grid, int tx, int ty, int ep, int io, hipStream_t st) {
    if (a.precision == PREC_F16X3) { if (ep == 0) HX_CO_IO(_Float16, 0); else if (ep == 1) HX_CO_IO(_Float16, 1); else return -1; }
    else if (a.precision == PREC_BF16X3) { if (ep == 2) HX_CO_IO(__bf16, 2); else if (ep == 0 && io == 0) HX_CO(__bf16, 0, 0); else if (ep == 0 && io == 1) HX_CO(__bf16, 0, 1); else return -1; }
    else return -1;
    return 1;
}

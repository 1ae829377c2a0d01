// Device-side JPEG reader (jpeg_read.hip): complete baseline JPEG files (8-bit, three components, 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan) back to back on the device ->
// uint8 interleaved frames where the frame pipeline (frames.hip) reads them.  What a JPEG-read context keeps besides the scaffold of eval_ctx.h.
#pragma once
#include "net.h"

struct JpegReadState {
    int max_frames = 0, H = 0, W = 0;
    int bw = 0, bh = 0;                      // the 8 x 8 blocks of a component plane padded to whole 2 x 2-block MCUs: 2 ceil(W / 16), 2 ceil(H / 16)
    long cstride = 0;                        // int16 coefficients between two images: 3 bw bh 64 (every sampling fits: the chroma planes are at most the luma's)
    long pstride = 0;                        // bytes between the component planes of two images: 3 (8 bh) (8 bw), a multiple of 64
};
void jpeg_read_free(caddy_ctx* c);      // releases caddy_ctx::jpeg_read (caddy_ctx_destroy)

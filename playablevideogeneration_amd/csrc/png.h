// Device-side PNG writer (png.hip): uint8 interleaved frames where the frame writer and the sheets left them -> complete PNG files (8-bit RGB, one IDAT), back to back.  What a
// PNG context keeps besides the scaffold of eval_ctx.h.
#pragma once
#include "net.h"

struct PngState {
    int max_frames = 0, H = 0, W = 0, filter_mode = 0;      // filter_mode: 0..4 one fixed filter type, 5 adaptive
    long stream = 0;                         // bytes of an image's filtered stream: H (1 + 3 W)
    long nb = 0;                             // deflate blocks per image: ceil(stream / PNG_BLOCK)
    long fstride = 0, cstride = 0;           // bytes between the filtered streams of two images / between the staged outputs of two blocks
    unsigned char head[41] = {};             // signature, IHDR, the IDAT length (filled on the device) and type
    unsigned char* d_head = nullptr;
    unsigned* d_crc_table = nullptr;         // 256 words: the reflected CRC-32 table; then 32 words: x^(2^k) mod P
};
void png_free(caddy_ctx* c);      // releases caddy_ctx::png (caddy_ctx_destroy)

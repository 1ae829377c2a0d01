// Device-side PNG reader (png_read.hip): complete PNG files (8-bit RGB, no interlace) back to back on the device -> uint8 interleaved frames where the frame pipeline
// (frames.hip) reads them.  What a PNG-read context keeps besides the scaffold of eval_ctx.h.
#pragma once
#include "net.h"

struct PngReadState {
    int max_frames = 0, H = 0, W = 0;
    long stream = 0;                         // bytes of an image's filtered stream: H (1 + 3 W)
    long capacity = 0;                       // IDAT bytes one image may hold (include/caddy_hip.h states the sum); more is CADDY_PNG_TOO_LARGE
    long zstride = 0, sstride = 0;           // bytes between the gathered IDAT bytes / the inflated streams of two images (multiples of 16)
    unsigned* d_crc_table = nullptr;         // 256 words: the reflected CRC-32 table; then 32 words: x^(2^k) mod P (as png.hip's)
};
void png_read_free(caddy_ctx* c);      // releases caddy_ctx::png_read (caddy_ctx_destroy)

// Device-side MJPEG writer (video.hip): uint8 interleaved frames where the frame writer left them -> complete baseline JPEG files, back to back.  What a VIDEO context keeps
// besides the scaffold of eval_ctx.h.
#pragma once
#include "net.h"

struct VideoState {
    int max_frames = 0, H = 0, W = 0, quality = 0;
    int mcux = 0, mcuy = 0, blocks = 0;      // MCUs per row / column of a frame; 8 x 8 blocks per frame (3 per MCU: Y, Cb, Cr)
    long wpf = 0, cpf = 0;                   // per frame: words of the bit buffer (its bound), chunks of VID_THREADS words
    unsigned char qt[128] = {};              // the two quantisation tables, natural order, luminance first
    std::vector<unsigned char> header;       // SOI .. SOS
    unsigned short* d_div = nullptr;         // 2 x 64 divisors (table << 3) in zigzag order
    unsigned* d_huff = nullptr;              // 4 x 256 (DC luminance, AC luminance, DC chrominance, AC chrominance): code | length << 16
    unsigned char* d_header = nullptr;
};
void video_free(caddy_ctx* c);      // releases caddy_ctx::vid (caddy_ctx_destroy)

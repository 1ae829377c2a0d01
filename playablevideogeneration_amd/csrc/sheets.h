// Evaluation example sheets (sheets.hip): fp32 planar frames where the forward pass left them -> one finished uint8 contact sheet.  What a SHEETS context keeps besides the scaffold of eval_ctx.h.
#pragma once
#include "net.h"

struct SheetsState {
    int max_rows = 0, max_cols = 0;      // the largest sheet a call may ask for: rows of cells (two per drawn sequence) x cells per row (sequence length)
    unsigned* d_words = nullptr;         // SH_WORDS device words: the flags of the reduction launch, the mask's maximum, the arrival counter, the counts and decisions of the last call
    unsigned* d_slab = nullptr;          // one partial maximum per wave of the reduction launch
};
void sheets_free(caddy_ctx* c);      // releases caddy_ctx::sh (caddy_ctx_destroy)

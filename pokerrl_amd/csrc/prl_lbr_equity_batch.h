// The check-down equities of MANY independent LBR decisions in one pass over the device (prl_lbr_equity_batch.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pokerrl_hip.h"

// device work buffers of the core; they only ever grow, so a caller that keeps one across calls (the batched engine: one per run) allocates once per size
struct PrlLbrEqWork {
    void* plan = nullptr;     // [cap_plan] PrlLbrEqPlan
    void* rec = nullptr;      // [cap_rec] PrlLbrEqRec
    uint16_t* lists = nullptr;  // [cap_lists] = requests x list stride
    float* eq = nullptr;      // [cap_eq] the (range, board) equities of a chunk
    size_t cap_plan = 0, cap_rec = 0, cap_lists = 0, cap_eq = 0;
};
void prl_lbr_eq_work_free(PrlLbrEqWork* w);

// n_req requests in the layout the batched engine's kernel writes: d_meta [n_req][8] (LBR's hand index, n_q, n_dealt, five table cards, -1 where none),
// d_ranges [n_req][q_stride][R], d_wp [n_req][q_stride] (slots at or beyond a request's n_q are not written). h_meta: the caller's host copy of d_meta
// (32 bytes per request: the chunks are planned from it). Everything is enqueued on `stream`; the call returns after ONE stream synchronisation,
// however many requests and chunks there were. out_chunks: how many passes over the equity buffer the memory budget (PRL_LBR_EQ_BATCH_MB) asked for.
int prl_lbr_equity_batch_device(const PrlRules* rules, int n_req, const int32_t* h_meta, const int32_t* d_meta, const float* d_ranges, int q_stride,
                                float* d_wp, void* stream, PrlLbrEqWork* work, int* out_chunks);

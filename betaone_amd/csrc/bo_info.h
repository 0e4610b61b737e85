// betaone_amd/csrc/bo_info.h -- what an interactive front end (betaone_amd/uci.py) needs from a FAST-mode search besides bo_step:
//
//   bo_k_fw_stop   one wave per game slot: end a running search between two steps.  The step in flight -- the rows bo_k_fw_select
//                  chose and bo_k_fw_leaf materialised, waiting for their evaluation -- is ABANDONED, not finished: nothing of it is
//                  in the tree.  The virtual loss is never written (bo_fastw.h: a step's descents read the tree only), the backup of a
//                  step's simulations happens in the NEXT select launch, and bo_k_fw_leaf writes the row's position, legal moves and
//                  planes, the control block's row_nlegal / row_term and the slot's evaluation counter -- no arena record.  So the tree
//                  and sims_done are those after the last completed backup; dropping the rows (FWC_NROWS = FWC_NSTEP = 0, req_node = -1)
//                  and marking the search finished is all there is to do.  Finishing the step instead would take another evaluation:
//                  a stop would cost a network forward.
//   bo_k_fw_info   one wave per game slot, READ-ONLY, whatever the phase: one fixed-size record per slot -- the search's state, the
//                  root children with the most visits (MultiPV lines) and the variation below each.  Enqueued between two steps, so
//                  the tree is at rest: every step's backup is complete, the step in flight has left nothing in it.
//
// No atomics; every loop is bounded: the line loop by BO_INFO_LINES, the walk by BO_INFO_PV, a scan by the run's records (a link
// names at most 128 granules; a link that does not lie inside the arena ends the walk).  Control flow is wave-uniform apart from
// lane-predicated stores.  bo_k_fw_info builds the record in LDS and stores every word of it exactly once: `out` may be pinned host
// memory that the host reads behind an event.
#pragma once
#include "bo_fastw.h"

// BO_INFO_LINES (8) and BO_INFO_PV (24) come from include/betaone_engine.h
#define BO_INFO_HEAD 16                                   // words in front of the lines
#define BO_INFO_LINE_WORDS 32                             // move, visits, w, prior, pv_len, pv[24], 3 reserved
#define BO_INFO_WORDS (BO_INFO_HEAD + BO_INFO_LINES * BO_INFO_LINE_WORDS)

BO_KERNEL void bo_k_fw_stop(Eng e, FastW f, const int *mask) {
    const int g = bo_block(), lane = bo_lane();
    if ((mask && !mask[g]) || e.phase[g] != PH_RUN) return;
    if (lane == 0) {
        int *ctl = fw_ctl(f, g);
        ctl[FWC_NROWS] = 0; ctl[FWC_NSTEP] = 0;
        e.req_node[g] = -1; e.phase[g] = PH_DONE;
    }
}

// the record with the most visits among the `nrec` records at R that come AFTER (pv, pk) in the order (visits descending, index
// ascending); (pv, pk) = (0x7fffffff, -1) for the first.  -> its index, *visits = its count (<= 0: none; padding has n = -1)
BO_DEV int info_next_best(const WRec *R, int nrec, int pv, int pk, int *visits) {
    int bv = -1, bk = 0x7fffffff;
    for (int i = bo_lane(); i < nrec; i += 64) {
        const int v = R[i].n;
        const bool after = v < pv || (v == pv && i > pk);
        if (after && v > bv) { bv = v; bk = i; }  // (a lane's indices ascend: the first maximum stays)
    }
    for (int m = 1; m < 64; m <<= 1) {
        const int ov = bo_shfl_xor(bv, m), ok = bo_shfl_xor(bk, m);
        if (ov > bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
    }
    *visits = bo_uniform(bv);
    return bo_uniform(bk);
}

// a link's run lies inside the arena (a corrupt link ends the walk instead of reading beyond it)
BO_DEV bool info_link_ok(const FastW &f, int link) {
    return link >= 0 && fw_first(link) >= 1 + BO_FW_HG && fw_first(link) + fw_ngran(link) <= f.NG;
}

// Words: 0 phase, 1 status, 2 terminal, 3 n_legal, 4 sims_done, 5 root_visits, 6 arena_top, 7 arena_granules, 8 the watched fault word
// as bo_k_fw_result left it, 9 n_lines, 10..15 zero; then BO_INFO_LINES lines of BO_INFO_LINE_WORDS words (include/betaone_engine.h).
BO_KERNEL void bo_k_fw_info(Eng e, FastW f, int n_want, int *out) {
    BO_SHARED int rec[BO_INFO_WORDS];
    const int g = bo_block(), lane = bo_lane();
    for (int i = lane; i < BO_INFO_WORDS; i += 64) rec[i] = 0;
    bo_sync();
    const int *ctl = fw_ctl(f, g);
    const WRec *A = fw_arena(f, g);
    const bo_mv *M = fw_moves(f, g);
    const int term = e.root_term[g], rlink = A[0].link;
    if (lane == 0) {
        rec[0] = e.phase[g]; rec[1] = e.status[g]; rec[2] = term; rec[3] = e.root_nlegal[g]; rec[4] = e.sims_done[g];
        rec[5] = A[0].n; rec[6] = ctl[FWC_TOP]; rec[7] = f.NG; rec[8] = e.res_watch[0];
    }
    int n_lines = 0;
    if (term == 0 && info_link_ok(f, rlink)) {
        const int want = n_want < BO_INFO_LINES ? n_want : BO_INFO_LINES;
        const size_t r0 = (size_t)fw_first(rlink) * BO_FW_GR;
        const int nrec0 = fw_ngran(rlink) * BO_FW_GR;
        int pv = 0x7fffffff, pk = -1;
        for (int l = 0; l < want; l++) {
            int v;
            const int k = info_next_best(A + r0, nrec0, pv, pk, &v);
            if (v <= 0) break;  // children without a visit are not lines
            pv = v; pk = k;
            int *ln = rec + BO_INFO_HEAD + l * BO_INFO_LINE_WORDS;
            size_t node = r0 + (size_t)k;
            if (lane == 0) {
                ln[0] = (int)M[node]; ln[1] = A[node].n; ln[2] = __builtin_bit_cast(int, A[node].w); ln[3] = __builtin_bit_cast(int, A[node].prior);
                ln[5] = (int)M[node];
            }
            int pv_len = 1;
            for (int d = 1; d < BO_INFO_PV; d++) {  // below: the child with the most visits, the first maximum in record order
                const int link = A[node].link;
                if (!info_link_ok(f, link)) break;  // unvisited, FW_MATE, FW_DRAW: no run
                const size_t c0 = (size_t)fw_first(link) * BO_FW_GR;
                int cv;
                const int ck = info_next_best(A + c0, fw_ngran(link) * BO_FW_GR, 0x7fffffff, -1, &cv);
                if (cv <= 0) break;
                node = c0 + (size_t)ck;
                if (lane == 0) ln[5 + d] = (int)M[node];
                pv_len++;
            }
            if (lane == 0) ln[4] = pv_len;
            n_lines++;
        }
    }
    if (lane == 0) rec[9] = n_lines;
    bo_sync();
    for (int i = lane; i < BO_INFO_WORDS; i += 64) out[(size_t)g * BO_INFO_WORDS + i] = rec[i];
}

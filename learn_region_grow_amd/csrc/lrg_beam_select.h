// The beam search's choice of the next queue (test_beam_search.py:282): Q = sorted(newQ, key=score, reverse=True)[:BEAM_WIDTH].
// One definition for the device (lrg_beam_advance_kernel, csrc/lrg_beam.inl) and the host (tools/beam_select_table.hip, which
// tests/test_beam_select.py runs): plain arrays in, no HIP call.
//
//   candidates  the children c with updated[c] == 1 (their mask changed, :275), in child order c = qid * SEARCH_WIDTH + search id
//   key         --scoring np: size[c] (points of the mask);  --scoring ml: score[c] (float64 log-likelihood; -inf is a legal score)
//   order       descending, STABLE: of two equal keys the earlier child stays first (Python's sorted; -inf == -inf is a tie)
//   best        the first beam_width of that order -- an emptied mask (size 0) takes its place here like any other entry ...
//   kept        ... and is dropped only afterwards (an emptied mask has no bounding box, oracle/beam_ref.py:140), so under 'ml',
//               where an emptied mask can carry a high score, the queue comes out shorter.  Under 'np' empties sort last, and
//               this equals excluding them before the selection.
#pragma once

#define LRG_BEAM_MAXQ 16      // BEAM_WIDTH <= 16, BEAM_WIDTH * SEARCH_WIDTH <= 64

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LRG_BEAM_HD __host__ __device__
#else
#define LRG_BEAM_HD
#endif

// best[0..n_best): the chosen children before the empties are dropped; kept[0..return): those of them with size > 0, same order.
// best and kept hold beam_width entries each (beam_width <= LRG_BEAM_MAXQ).
LRG_BEAM_HD inline int lrg_beam_select(int n_children, const int *updated, const int *size, const double *score, int scoring_ml,
                                       int beam_width, int *best, int *n_best, int *kept) {
    int nb = 0;
    for (int c = 0; c < n_children; ++c) {
        if (updated[c] != 1) continue;
        int k = nb < beam_width ? nb : beam_width;                       // insertion into the best-beam_width list, from its end
        while (k > 0 && (scoring_ml ? score[best[k - 1]] < score[c] : size[best[k - 1]] < size[c])) {
            if (k < beam_width) best[k] = best[k - 1];
            --k;
        }
        if (k < beam_width) { best[k] = c; if (nb < beam_width) ++nb; }
    }
    int nk = 0;
    for (int k = 0; k < nb; ++k)
        if (size[best[k]] > 0) kept[nk++] = best[k];
    *n_best = nb;
    return nk;
}

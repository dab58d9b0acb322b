// probe_fit_walk.inc -- the walk of a fit kernel up to its residual stage, included behind probe_fit_setup.inc and the kernel's own
// per-thread state: persistent workgroups take the 32-row tiles of X in turn, the next tile (and its rows' labels) in flight under this
// tile's arithmetic; per tile phase 1 (scores), then the residual stage opens -- the kernel's own text follows this file and
// probe_fit_rest.inc closes it.  The including kernel provides, besides the names of probe_fit_setup.inc,
//   y                      the labels [N]
//   row_fetch(h, gr)       a lambda: loads whatever else the residual of row gr (half h of a coming tile) needs; runs with the label prefetch
//   row_latch()            a lambda: moves what row_fetch loaded to where the residual stage reads it, before the next tile's fetch overwrites it
// (both empty where the label is all a row needs) and its residual stage, one pass per half tile h, which reads r (the row in the tile),
// gr (the row in X), ycur[h] (its label, -1 past N) and zp through join_scores(zp, r * kGroup + rc, bias), and leaves `float res`: the
// residual of (row, this thread's problem), 0 for a dead column or row.  Every thread runs it (the softmax shuffles across lanes).  The
// residual stage is text and not a third lambda: as a lambda it changed the kernels' instructions.
  // D <= 512: the next tile waits in registers while this one is computed; wider rows need those registers for wf and g
  constexpr bool kPrefetch = CT <= 8;
  T tile;
  long t = blockIdx.x;
  int ynext[2] = {-1, -1};
  auto fetch = [&](long tl) {
    if constexpr (kPrefetch) tile.fetch(X, N, D, tl * kRows, tid);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long gr = tl * kRows + rr + 16 * h;
      ynext[h] = gr < N ? y[gr] : -1;
      row_fetch(h, gr);
    }
  };
  if (t < ntiles) fetch(t);
  while (t < ntiles) {
    if constexpr (kPrefetch) tile.stage(xs, tid); else T::direct(X, N, D, t * kRows, tid, xs);
    const int ycur[2] = {ynext[0], ynext[1]};
    row_latch();
    __syncthreads();
    const long next = t + gridDim.x;
    if (next < ntiles) fetch(next);     // in flight under this tile's arithmetic
    T::scores(xs, wf, zp, wave, lane);
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = rr + 16 * h;
      const long gr = t * kRows + r;

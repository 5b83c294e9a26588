// The frame of a row under RANGE BETWEEN x PRECEDING / FOLLOWING AND y PRECEDING / FOLLOWING (tgpu_window_factory_create_ranged): the closed form
// of the reference's stateful walk (getFrameRange / seek, M/operator/window/WindowPartition.java:325-521, emptyFrame :523-528).
//
// This text has no #include and uses plain int / long long / unsigned long long only: window.hip compiles it for the device and a host program
// (tests/range_frame/range_main.cpp) compiles it as it stands and checks it on the CPU under the sanitizers.  Every function is declared through
// TG_RANGE_FN.
//
// All indices are positions of the sorted order.  A row's partition is [ps, pe], its peer group [peer_s, peer_e].  `codes` holds, per position, the
// comparison key as an order-preserving unsigned 64-bit code, COMPLEMENTED under a descending sort, so that in a partition's run of non-null sort
// keys [lo, hi] the codes never decrease and "K[p] precedes or equals the bound B" is codes[p] <= code(B), whatever the type and the direction.
// Nothing here reads `codes` outside [lo, hi], and [lo, hi] is inside [ps, pe]: a comparison key that is not monotone gives some frame inside the
// partition, never an index outside it.
#ifndef TG_RANGE_FRAME_HELPERS
#define TG_RANGE_FRAME_HELPERS
#if defined(__HIPCC__)   // both passes of the HIP compiler; a plain host compiler takes the other branch
#define TG_RANGE_FN static __host__ __device__ __forceinline__
#else
#define TG_RANGE_FN static inline
#endif

// sql/tree/FrameBound.Type ordinals (tgpu_frame_bound)
#define TG_RANGE_UNBOUNDED_PRECEDING 0
#define TG_RANGE_PRECEDING 1
#define TG_RANGE_CURRENT_ROW 2
#define TG_RANGE_FOLLOWING 3
#define TG_RANGE_UNBOUNDED_FOLLOWING 4

// The partition's run of non-null sort keys.  With ONE sort channel the partition's null keys are one peer group (null is not distinct from
// null) at its head (nulls first) or its tail: the run is what the first / last row's peer group leaves.  first_null / last_null = the sort key
// of row ps / pe is null, first_peer_e = the last peer of row ps, last_peer_s = the first peer of row pe.  An all-null partition: lo > hi.
TG_RANGE_FN void tg_range_run(int nulls_first, long long ps, long long pe, int first_null, long long first_peer_e, int last_null, long long last_peer_s,
                              long long *lo, long long *hi)
{
  long long l = ps, h = pe;
  if (nulls_first) {
    if (first_null) l = first_peer_e + 1;
  }
  else if (last_null) {
    h = last_peer_s - 1;
  }
  // held inside the partition whatever the peer arrays say
  if (l < ps) l = ps;
  if (h > pe) h = pe;
  *lo = l;
  *hi = h;
}

TG_RANGE_FN int tg_range_behind(unsigned long long code, unsigned long long bound, int strict) { return strict ? code > bound : code >= bound; }

// The first p of [lo, hi] with codes[p] >= bound (strict: > bound), hi + 1 if there is none; lo <= at <= hi is where the search sets out (the
// row's own position).  It gallops outward from `at` in steps of 1, 2, 4 .. and bisects the last step, so the reads follow log2 of the distance
// from the row to its bound, not log2 of the partition.  Never reads outside [lo, hi].
TG_RANGE_FN long long tg_range_first(const unsigned long long *codes, long long lo, long long hi, long long at, unsigned long long bound, int strict)
{
  if (lo > hi) return hi + 1;
  if (at < lo) at = lo;
  if (at > hi) at = hi;
  long long below, above;   // codes[below] is in front of the bound (or below = lo - 1), codes[above] is behind it (or above = hi + 1)
  if (tg_range_behind(codes[at], bound, strict)) {
    above = at;
    below = lo - 1;
    for (long long step = 1; at - step >= lo; step += step) {
      if (!tg_range_behind(codes[at - step], bound, strict)) {
        below = at - step;
        break;
      }
      above = at - step;
    }
  }
  else {
    below = at;
    above = hi + 1;
    for (long long step = 1; at + step <= hi; step += step) {
      if (tg_range_behind(codes[at + step], bound, strict)) {
        above = at + step;
        break;
      }
      below = at + step;
    }
  }
  while (above - below > 1) {
    const long long mid = below + (above - below) / 2;   // lo <= mid <= hi
    if (tg_range_behind(codes[mid], bound, strict)) above = mid;
    else below = mid;
  }
  return above;
}

// The frame [*s, *e] of row i; returns 0 for an empty frame (then *s = *e = -1).
//   a row whose sort key is null    its peer group, stretched to the partition's first / last row by UNBOUNDED_*; no bound is read
//   otherwise                       start with a value: the first p of [lo, hi] with B <= K[p], else hi + 1;  end with a value: the last p of
//                                   [lo, hi] with K[p] <= B, else lo - 1;  CURRENT_ROW: the peer group;  UNBOUNDED_*: the partition
//   empty (emptyFrame, :523-528)    start > end, start behind the partition, end in front of it
// start_codes / end_codes are read for a PRECEDING / FOLLOWING bound of a non-null row only.
TG_RANGE_FN int tg_range_frame(int start_type, int end_type, long long i, long long ps, long long pe, long long peer_s, long long peer_e, int row_null, long long lo,
                               long long hi, const unsigned long long *start_codes, unsigned long long start_bound, const unsigned long long *end_codes,
                               unsigned long long end_bound, long long *s, long long *e)
{
  long long a, b;
  if (row_null) {
    a = start_type == TG_RANGE_UNBOUNDED_PRECEDING ? ps : peer_s;
    b = end_type == TG_RANGE_UNBOUNDED_FOLLOWING ? pe : peer_e;
  }
  else {
    if (start_type == TG_RANGE_UNBOUNDED_PRECEDING) a = ps;
    else if (start_type == TG_RANGE_CURRENT_ROW) a = peer_s;
    else a = tg_range_first(start_codes, lo, hi, i, start_bound, 0);
    if (end_type == TG_RANGE_UNBOUNDED_FOLLOWING) b = pe;
    else if (end_type == TG_RANGE_CURRENT_ROW) b = peer_e;
    else b = tg_range_first(end_codes, lo, hi, i, end_bound, 1) - 1;
  }
  if (a > b || a > pe || b < ps || a < ps || b > pe) {
    *s = *e = -1;
    return 0;
  }
  *s = a;
  *e = b;
  return 1;
}
#endif

// device_fq_args.h -- FqArgs, the argument block of the one-pass aggregation kernels (fq_onepass, fq_onepass_multi).
// This is the only definition: the host includes this file (jit.h) and the fused aggregations with group-by keys embed it verbatim.
// Needs device_fa_args.h and device_cols.h (TgKeyCols) before it.
#pragma once

struct FqArgs {
  FaArgs fa;
  TgKeyCols store;
  int store_groups;
  int pad;
  unsigned long long* counters;        // this page: [0] rows of unknown groups, [7] expression error word (~0 = none)
  const unsigned long long* prev;      // the previous one-pass page's counters (its totals are in fold.pending), or null
  unsigned long long* host_out;        // host-visible words for the counters ({[0], [2], [7]}, then a flag in word 7), written by the
  unsigned int* done;                  // workgroup that finishes last (`done` = finished workgroups, rests at 0); null: the host copies
  const FpArgs* pages;                 // fq_onepass_multi: the launch's pages in order (device memory; error words all = fa.fp.error)
  int n_pages;
  int pad3;
};

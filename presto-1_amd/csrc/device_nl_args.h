// device_nl_args.h -- NlArgs, the argument block of the nested-loop filter kernels (nlj_pair_count, nlj_pair_emit).
// This is the only definition: the host includes this file (jit.h) and the nested-loop filter's generated sources embed it verbatim.
// Needs device_fp_args.h before it.
#pragma once

#define NL_STRIP 32   // small rows one wave evaluates for its 64 large rows
struct NlArgs {
  FpArgs fp;
  unsigned long long* masks;
  int* counts;
  const int* offsets;
  int* pair_probe;
  int* pair_build;
  long long s0, S;     // rows [s0, s0 + S) of the small side ...
  long long l0, Ln;    // ... against rows [l0, l0 + Ln) of the large side
  long long W;         // waves over the large rows: ceil(Ln / 64)
  int build_large, pad;
};

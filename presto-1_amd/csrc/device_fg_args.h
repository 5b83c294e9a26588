// device_fg_args.h -- FgArgs, the argument block of the fused filter + group-by probe kernel (fg_probe).
// This is the only definition: the host includes this file (jit.h) and the fused aggregations with group-by keys embed it verbatim.
// Needs device_fp_args.h and device_cols.h (TgKeyCols) before it.
#pragma once

struct FgArgs {
  FpArgs fp;
  TgKeyCols store;
  unsigned long long* words;
  unsigned long long mask;
  int* out;
  unsigned long long* counters;
  long long row0;
  long long n;
  int store_groups;
  int pad;
  const FgArgs* self;      // device copy of this block, read by the out-of-line table path (null: the kernel takes the kernarg segment)
  unsigned char* out8;     // compact mode: one byte per row instead of `out` (GbhProbeLaunch)
};

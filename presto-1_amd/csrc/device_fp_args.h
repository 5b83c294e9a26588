// device_fp_args.h -- FpArgs, the argument block of the generated filter + project kernels (fp_count, fp_emit), which every other fused
// kernel's block embeds, with its limits and the expression error codes.  This is the only definition: the host includes this file
// (jit.h) and every generated source embeds it verbatim.  Self-contained.
#pragma once

#define TG_E_RANGE 2
#define TG_E_DIV0 7
#define TG_E_CAST 9
#define TG_E_CONCAT 10
#define TG_E_ABS_BIGINT 11
#define TG_E_ABS_INTEGER 12
#define TG_E_ROUND 13
#define TG_MAXC 24   // input channels
#define TG_MAXP 16   // computed projections
struct FpArgs {
  const void* col_values[TG_MAXC];
  const unsigned char* col_nulls[TG_MAXC];
  const int* col_offsets[TG_MAXC];
  void* out_values[TG_MAXP];
  unsigned char* out_nulls[TG_MAXP];
  int* positions;
  const int* tile_offsets;
  int* tile_counts;
  unsigned long long* error;
  long long n;
  unsigned long long* sel_mask;   // filter verdicts of pass 1, one 64-bit ballot per (tile, stripe, wave)
  long long* operand;             // null, or where the lane that posts operand_key stores the operand of its failure (jit.cpp raise_operand)
  unsigned long long operand_key;
};

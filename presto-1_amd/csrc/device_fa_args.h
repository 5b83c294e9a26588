// device_fa_args.h -- FaArgs, the argument block of the fused project + accumulate kernels (fa_mask, fa_accumulate_*, fa_ordered_chain).
// This is the only definition: the host includes this file (jit.h) and the fused aggregation's generated sources embed it verbatim.
// Needs device_fp_args.h and device_agg.h before it.
#pragma once

struct FaArgs {
  FpArgs fp;
  const int* gids;
  unsigned char* mask_out;
  TgAggState st[TG_MAX_AGGS];
  TgLowCardPlan plan;
  long long tiles;
  int lowcard;
  int pad;
  const unsigned int* ord_keys;   // ORDERED mode: (group id + 1) of the page's rows in (group, row) order, 0 = filtered row
  const int* ord_rows;            //               and their row numbers
  const unsigned char* gids8;     // compact group ids (id + 1, 0 = filtered row) instead of gids
  TgFoldScratch fold;             // low-cardinality launches: the workgroups' folded partials
  const unsigned long long* gate; // speculative launch behind a group-by probe: its counters; anything but clean = do nothing
  const int* ord_stretch;         // ORDERED mode, chained kernel over all groups: {first, end} of every group's stretch of ord_keys; or
  long long* ord_list;            // the groups the lane-per-group kernel handed over after ord_handoff rows: {group, next index} pairs,
  unsigned int* ord_list_count;   // their number (starts at 0); ord_handoff 0 = lanes walk their groups to the end
  int ord_handoff;
  int pad4;
  unsigned long long* spill_dirty; // one-pass launches (totals pending): a residue of the lane-private pairs counts here and makes the page
                                   // dirty; null = the residues go straight to the limbs (device_agg.h TgSpill)
};

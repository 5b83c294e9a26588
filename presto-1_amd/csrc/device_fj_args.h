// device_fj_args.h -- FjArgs and FjPairArgs, the argument blocks of the fused filter + project + probe kernels (fj_probe, fj_emit, fj_pair).
// This is the only definition: the host includes this file (jit.h) and the fused probe's generated sources embed it verbatim.
// Needs device_fp_args.h and device_join.h before it.
#pragma once

#define FJ_COUNT_SLOTS 64      // words the workgroups of pass 1 spread their selected-row counts over
#define FJ_MAX_BUILD_COLS 4    // build-side output channels pass 2 gathers itself
#define FJ_MAX_CARRY 4         // probe-side output channels pass 1 can carry
// a build-side output channel gathered by pass 2 itself (fixed-width columns; one launch instead of one more per channel)
struct FjBuildCol {
  const void* values;
  const unsigned char* nulls;
  void* out_values;
  unsigned char* out_nulls;
  int width;
  int pad;
};
struct FjArgs {
  FpArgs fp;
  const TgSlot16* slots;
  unsigned long long mask;
  TgPrefilter pf;
  int* tile_cnt;            // pairs produced by each CHUNK of tiles (see fj_probe)
  int* tile_src;            // where the chunk's pairs start inside its block's private region
  const int* tile_dst;      // pass 2: exclusive scan of tile_cnt = final output offset of the chunk
  int* pair_probe;          // block-private regions, capacity = rows the block owns
  int* pair_build;
  int* out_build;           // pass 2: build positions in final order
  unsigned long long* counters;   // [0] rows selected by the filter
  long long tiles;
  long long grid1;          // grid size of pass 1 (defines the region layout)
  int outer;                // bit 0: PROBE_OUTER / FULL_OUTER rows; bit 1: nobody reads the build positions (no build output channels,
                            // no outer tracking): the DIRECT layout then skips the rank and position lookups
  int chunk_shift;          // a workgroup takes 2^chunk_shift consecutive tiles at a time
  FjBuildCol bcol[FJ_MAX_BUILD_COLS];
  int n_bcol;
  int pad2;
  void* carry[FJ_MAX_CARRY];  // FJ_CARRY: block-private regions of the probe-side output VALUES, one per output channel (pass 1 evaluates
                              // them from its row registers for every emitted pair; pass 2 moves them instead of re-reading the input
  unsigned char* carry_nulls; // columns sparsely), and of their null bits (nullptr: no output can be null)
  unsigned long long* host_out; // epilogue (small pages): host-visible result words {error, pairs, selected}, written by the LAST workgroup
                                // of pass 1 after it has scanned the chunk counts (null: none)
  unsigned int* done;           //                         workgroups that have finished (rests at 0)
  const FpArgs* pages;          // FJ_EPILOGUE == 2 (a launch over a LIST of pages): one FpArgs per page, in device memory
  const int* page_tile0;        //   first tile of each page in the launch's tile sequence, [n_pages] = all tiles
  int n_pages;
  int pad3;
};
// fj_pair: pass 1 of one page (the first probe_blocks workgroups) and pass 2 of an earlier page in one launch
struct FjPairArgs {
  FjArgs probe;
  FjArgs emit;
  unsigned int probe_blocks;
  unsigned int pad;
};

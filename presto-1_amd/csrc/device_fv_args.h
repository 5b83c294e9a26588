// device_fv_args.h -- FvArgs, the argument block of fp_vwrite, the write pass of the computed VARCHAR projections: fp_emit left each row's
// byte length in out_values[slot] (an int32 array), the scan of it is offsets[v], and the kernel evaluates the projection again to copy its
// bytes to pool[v] + offsets[v][o].  The block is this kernel's own: FpArgs, which every fused kernel embeds, keeps its layout.
// This is the only definition: the host includes this file (jit.h) and the page processors with computed VARCHAR projections embed it
// verbatim.  Needs device_fp_args.h before it.
#pragma once

#define TG_MAXV 8   // computed VARCHAR projections of one page processor
struct FvArgs {
  FpArgs fp;
  const int* offsets[TG_MAXV];
  unsigned char* pool[TG_MAXV];
  long long n_out;
};

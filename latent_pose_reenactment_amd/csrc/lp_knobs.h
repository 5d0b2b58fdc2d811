// Every environment switch of the kernel dispatchers: one line per knob (field, name, default, meaning), read once per process on the
// first lp_knobs() call.  Host-only: nothing from HIP is included.
#pragma once
#include <stdlib.h>

static inline int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }

struct LpKnobs {
    int conv_pp          = env_int("LP_CONV_PP", -1);           // -1: auto (ping-pong when the paired grid covers the chip); 0 | 1: force off | on
    int conv_w8          = env_int("LP_CONV_W8", -1);           // -1: auto (8-wave groups on maps of <= 256 pixels); 0 | 1: force off | on
    int conv_ksplit      = env_int("LP_CONV_KSPLIT", 8);        // largest split-K factor of the 3x3 convs
    int conv_split_wgs   = env_int("LP_CONV_SPLIT_WGS", 256);   // split K while at most this many workgroups result
    int conv_nbuf        = env_int("LP_CONV_NBUF", 0);          // 0: auto (3-deep weight ring on grids of <= 320 workgroups); 2 | 3: force
    int conv_xcd         = env_int("LP_CONV_XCD", 1);           // 1: XCD-ordered conv grids; 0: plain 2-D grid; 2: 1-D grid in plain order (debug)
    int conv_pipe        = env_int("LP_CONV_PIPE", 1);          // 1: conv_pipe_kernel takes the 3x3 layers it covers; 0: off
    int conv_pipe_mr     = env_int("LP_CONV_PIPE_MR", 0);       // 0: auto; 4 | 8: force its rows per wave at any grid size, and admit bf16x3 (tests)
    int conv1x1_pipe     = env_int("LP_CONV1X1_PIPE", 0);       // 0: off; 1: conv1x1_pipe_kernel on the layers it was built for; 2: every shape (tests)
    int wgrad_cob        = env_int("LP_WGRAD_COB", 0);          // 0: auto = 128 output channels per workgroup of the 3x3 conv_wgrad_kernel; 64 | 128: force
    int wgrad3_pipe      = env_int("LP_WGRAD3_PIPE", 1);        // 1: wgrad3_pipe_kernel for layers with enough pixel tiles; 0: never; 2: every 3x3 layer (tests)
    int wgrad3_x3        = env_int("LP_WGRAD3_X3", 1);          // 1: dense bf16x3 layers on wgrad3_pipe_kernel; 0: on conv_wgrad_kernel
    int thin_mfma        = env_int("LP_THIN_MFMA", 1);          // 1: RGB -> 64 k-channel 3x3 convs on the MFMA kernel; 0: fp32 VALU kernel always
    int gconv_rows       = env_int("LP_GCONV_ROWS", 1);         // 1: gconv_rows_kernel on whole 4 x 16 tiles; 0: conv_dma_kernel; 2: every shape it can express
    int gconv_rows_wgs   = env_int("LP_GCONV_ROWS_WGS", 0);     // 0: no cap; n: at most n workgroups per channel block
    int stat_split_fixed = getenv("LP_STAT_SPLIT_FIXED") != nullptr;      // unset -> 0: adaptive stage-1 split; set to ANYTHING -> 1: fixed 1024 pixels
};

inline const LpKnobs& lp_knobs() { static const LpKnobs k; return k; }

// Host-side record of the form the conv and weight-gradient dispatchers chose for the calling thread's last launch: which kernel, which
// template instance, which schedule (include/lp_hip.h: lp_last_launch_form).  Tests read it to assert the form their ids name.  Host-only:
// nothing from HIP is included, no kernel reads it; the launch functions fill it after their decisions are made.
#pragma once
#include <string.h>

#define LP_FORM_INTS 20
// slot 0: what the record describes; slot 1: the kernel; slot 19: precision mode
enum { LP_FORM_NONE = 0, LP_FORM_CONV = 1, LP_FORM_WGRAD = 2 };
enum { LP_FORM_CONV_DMA = 1, LP_FORM_CONV_PIPE = 2, LP_FORM_CONV_PIPE1X1 = 3 };
enum { LP_FORM_WGRAD_GENERIC = 1, LP_FORM_WGRAD_1X1 = 2, LP_FORM_WGRAD_PIPE3 = 3 };
enum { LP_FORM_WRED_TILED = 1, LP_FORM_WRED_FLAT32 = 2, LP_FORM_WRED_FLAT256 = 3 };
// conv slots
enum { LP_FC_KS = 2, LP_FC_UPS, LP_FC_WM, LP_FC_WN, LP_FC_MR, LP_FC_NR, LP_FC_CC, LP_FC_PP, LP_FC_NBUF, LP_FC_KSPLIT, LP_FC_ADBUF, LP_FC_STATS,
       LP_FC_FINISH, LP_FC_TILES, LP_FC_LTH, LP_FC_LTW, LP_FC_LNB };
// weight-gradient slots
enum { LP_FW_KS = 2, LP_FW_UPS, LP_FW_COB, LP_FW_SPLITS, LP_FW_RED, LP_FW_BIAS, LP_FW_TILES, LP_FW_LTH, LP_FW_LTW, LP_FW_LNB };
#define LP_FORM_PREC 19

int* lp_form_record();      // the calling thread's record (lp_api.hip)

static inline int* lp_form_begin(int what, int kernel, int prec) {
    int* f = lp_form_record();
    memset(f, 0, LP_FORM_INTS * sizeof(int));
    f[0] = what; f[1] = kernel; f[LP_FORM_PREC] = prec;
    return f;
}

// P: Conv16Params after the launcher has settled tiling, split and statistics
template <class P>
static inline void lp_form_conv(int kernel, int prec, int ks, int ups, int wm, int wn, int mr, int nr, int cc, int pp, int nbuf, const P& p) {
    int* f = lp_form_begin(LP_FORM_CONV, kernel, prec);
    f[LP_FC_KS] = ks; f[LP_FC_UPS] = ups; f[LP_FC_WM] = wm; f[LP_FC_WN] = wn; f[LP_FC_MR] = mr; f[LP_FC_NR] = nr; f[LP_FC_CC] = cc;
    f[LP_FC_PP] = pp; f[LP_FC_NBUF] = nbuf; f[LP_FC_KSPLIT] = p.ksplit; f[LP_FC_ADBUF] = p.a_dbuf; f[LP_FC_STATS] = p.stats ? 1 : 0;
    f[LP_FC_TILES] = p.ntiles; f[LP_FC_LTH] = p.lTH; f[LP_FC_LTW] = p.lTW; f[LP_FC_LNB] = p.lNB;
}

// P: WgradParams after the launcher has settled tiling and splits (the reduction form is added by launch_wreduce)
template <class P>
static inline void lp_form_wgrad(int kernel, int prec, int ks, int ups, int cob, int tiles, int lth, int ltw, int lnb, const P& p) {
    int* f = lp_form_begin(LP_FORM_WGRAD, kernel, prec);
    f[LP_FW_KS] = ks; f[LP_FW_UPS] = ups; f[LP_FW_COB] = cob; f[LP_FW_SPLITS] = p.splits; f[LP_FW_BIAS] = p.bpart ? 1 : 0;
    f[LP_FW_TILES] = tiles; f[LP_FW_LTH] = lth; f[LP_FW_LTW] = ltw; f[LP_FW_LNB] = lnb;
}

// error plumbing of the C ABI
#include "lp_hip.h"
#include "lp_internal.h"
#include "lp_launch_form.h"
#include <stdio.h>
#include <string.h>

static thread_local char g_err[512] = "";

int lp_set_error(int code, const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

int lp_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: launch failed: %s", what, hipGetErrorString(e));
        return LP_ERR_HIP;
    }
    return LP_OK;
}

extern "C" const char* lp_last_error(void) { return g_err; }
extern "C" int lp_abi_version(void) { return 12; }

static thread_local int g_form[LP_FORM_INTS] = {0};
int* lp_form_record() { return g_form; }

extern "C" int lp_last_launch_form(int* out, int capacity) {
    if (!out) return lp_set_error(LP_ERR_ARG, "lp_last_launch_form: null pointer");
    if (capacity < LP_FORM_INTS) return lp_set_error(LP_ERR_ARG, "lp_last_launch_form: capacity below the record's 20 ints");
    memcpy(out, g_form, sizeof(g_form));
    return LP_OK;
}

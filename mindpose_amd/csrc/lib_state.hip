// The library's per-thread state (last HIP error, the dry-launch switch of the acceptance queries), version and error strings.
#include "common.h"

namespace mp {

thread_local int g_last_hip_error = 0;
thread_local bool g_dry_launch = false;

}  // namespace mp

using namespace mp;

extern "C" {

const char* mp_version(void) { return "mindpose_hip 0.4.0 (gfx950)"; }

const char* mp_error_string(int code) {
    switch (code) {
        case MP_OK: return "ok";
        case MP_ERR_NULL: return "required pointer is NULL";
        case MP_ERR_SHAPE: return "bad shape";
        case MP_ERR_UNSUPPORTED: return "unsupported configuration";
        case MP_ERR_HIP: return "HIP runtime error";
        case MP_ERR_WORKSPACE: return "workspace missing or too small";
        default: return "unknown error";
    }
}

int mp_last_hip_error(void) { return g_last_hip_error; }

}  // extern "C"

// abi.hip -- the library-wide entries of include/ct_hip.h: ABI version, sticky device status, error text.  Host code only.
#include <hip/hip_runtime.h>

#include "../../include/ct_hip.h"
#include "ct_conv.h"
#include "ct_reinhard_persist.h"

extern "C" {

int ct_abi_version(void) { return CT_ABI_VERSION; }

int ct_device_status(int clear) {
    const int a = ct::rp::read_status(clear != 0), b = ct::conv_split_read_status(clear != 0);
    if (a < 0 || b < 0) return -1;
    return a | (b << 1);
}

const char *ct_error_string(int code) {
    switch (code) {
        case CT_OK: return "ok";
        case CT_E_BADARG: return "bad argument (null pointer, negative size or unknown enum)";
        case CT_E_WORKSPACE: return "workspace missing, misaligned or smaller than ct_workspace_bytes()";
        case CT_E_ALIGN: return "image pointer not aligned to its element size";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown ct error";
    }
}

}  // extern "C"

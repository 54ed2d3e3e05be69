// ABI bookkeeping of librgda_hip.so.
#include "common.h"

extern "C" int rgda_abi_version(void) { return RGDA_ABI_VERSION; }

extern "C" size_t rgda_class_lds(int which, int c, int n, int W) {
    switch (which) {
        case RGDA_LDS_LOSS_ROW: return loss_row_lds_bytes(c, n, W, true);
        case RGDA_LDS_PCL: return pcl_lds_bytes(c, n);
        case RGDA_LDS_REFINE: return refine_lds_bytes(c, n);
        default: return 0;
    }
}

extern "C" size_t rgda_class_lds_limit(int which) {
    switch (which) {
        case RGDA_LDS_LOSS_ROW: return RGDA_LOSS_ROW_LDS_MAX;
        case RGDA_LDS_PCL:
        case RGDA_LDS_REFINE: return RGDA_LDS_MAX;
        default: return 0;
    }
}

extern "C" const char* rgda_strerror(int status) {
    switch (status) {
        case RGDA_OK: return "ok";
        case RGDA_ERR_ARG: return "invalid argument (null pointer, bad shape or unsupported parameter value)";
        case RGDA_ERR_WORKSPACE: return "workspace too small";
        case RGDA_ERR_LAUNCH: return "HIP launch failed";
        case RGDA_ERR_UNSUPPORTED: return "configuration not supported by this build";
        default: return "unknown status";
    }
}

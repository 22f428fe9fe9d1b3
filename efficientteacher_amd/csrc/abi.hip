// Library identification entry points of the C ABI (include/et_hip.h), and the record of the environment's ET_* knobs.
#include "et_device.h"
#include "../../include/et_hip.h"
#include <stdio.h>
#include <stdlib.h>

extern "C" const char* et_build_arch(void) { return "gfx950"; }
extern "C" int et_abi_version(void) { return ET_ABI_VERSION; }

extern "C" int et_env_knobs(char* buf, int buflen) {
    // every ET_* runtime knob that is SET in this process's environment, as "NAME=value;..." (bench.py records it).  The complete list:
    // three test hooks (persistent-grid sizes, the BatchNorm finalize form), the switch back from buffer-descriptor LDS-DMA (the default of conv_gemm_pprs_kernel, conv_gemm_rs_kernel, conv1x1_stream_kernel and the 1x1 weight gradient) to the flat-address twins, the opt-in arms that change WHAT runs beside what (step
    // graph, weight-gradient stream, the stem on uint8 planes or on the packed image), the data-parallel transport settings, and the experiment-library path.
    static const char* names[] = {"ET_CONV_S1_WGS", "ET_CONV_STEM_WGS", "ET_CONV_BUF_DMA", "ET_BN_FIN_SMALL", "ET_STEP_GRAPH", "ET_WGRAD_STREAM", "ET_STEM_U8",
                                  "ET_ALLREDUCE_CHUNK_MB", "ET_ALLREDUCE_DTYPE", "ET_RCCL_CHANNELS", "ET_DP_SINGLE_RANK", "ET_HIP_LIB"};
    if (!buf || buflen < 1) return -1;
    int off = 0;
    buf[0] = 0;
    for (const char* n : names) {
        const char* v = getenv(n);
        if (!v) continue;
        const int w = snprintf(buf + off, buflen - off, "%s=%s;", n, v);
        if (w < 0 || w >= buflen - off) return -3;
        off += w;
    }
    return 0;
}

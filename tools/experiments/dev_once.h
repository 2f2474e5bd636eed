// The per-device "done once" bookkeeping these retired kernels' launchers were written against (the library's launchers use
// csrc/launch.h's DeviceSetup instead).  Plain flags: fine for the single-threaded probes that include these files.
#pragma once
#include "launch.h"

struct DevOnce {
    bool done[HIPT_MAX_DEV] = {};
    int ncu[HIPT_MAX_DEV] = {};
};
inline int hipt_cur_device() {
    int d = 0;
    return (hipGetDevice(&d) == hipSuccess && d >= 0 && d < HIPT_MAX_DEV) ? d : -1;
}
#define HIPT_CUR_DEVICE(dev)                                              \
    const int dev = hipt_cur_device();                                    \
    if (dev < 0) {                                                        \
        hipt_set_error("%s:%d: hipGetDevice failed", __FILE__, __LINE__); \
        return HIPT_E_LAUNCH;                                             \
    }

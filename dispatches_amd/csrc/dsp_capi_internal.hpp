// dsp_capi_internal.hpp — shared by dsp_capi.hip and dsp_capi_loop.hip: the thread's last HIP error (dsp_last_hip_error) and HIP_TRY, which records it
#pragma once
#include "dsp_device.hpp"

namespace dsp { inline thread_local int g_last_hip_error = 0; }

#define HIP_TRY(expr)                                                                                            \
  do {                                                                                                           \
    if (hipError_t _e = (expr); _e != hipSuccess) { dsp::g_last_hip_error = (int)_e; return DSP_ERR_HIP; }       \
  } while (0)

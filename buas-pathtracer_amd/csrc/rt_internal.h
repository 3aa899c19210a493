// Host helpers that rt_kernels.hip exports to the library's other translation units.
// Not part of the C ABI (include/rt_abi.h): C++ linkage, no header outside csrc/ names them.
#ifndef RT_INTERNAL_H
#define RT_INTERNAL_H

#include "rt_abi.h"

void rt_internal_set_error(const char* message);        // the thread's rt_last_error() message
int  rt_internal_bind_device(int device);               // hipSetDevice with the ABI's checks: an rt_status
int  rt_internal_scene_device(const rt_scene* scene);   // the device rt_scene_upload put the scene on
int  rt_internal_scene_cancelled(const rt_scene* scene); // rt_cancel's flag: set until the next frame's loop starts

#endif

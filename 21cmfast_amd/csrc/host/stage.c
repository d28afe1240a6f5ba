/*
 * stage.c -- staging of host arrays through workspace slots, shared by every host driver.
 */
#include "../hip/c21hip.h"
#include "c21cm_grid.h"

const void *c21_stage_in(int slot, const void *p, size_t bytes, void *stream, int *status) {
    if (!p || *status) return NULL;
    if (c21hip_is_device_ptr(p)) return p;
    void *d = c21hip_ws(slot, bytes);
    if (!d) {
        *status = C21CM_MEMORY_ALLOC_ERROR;
        return NULL;
    }
    int st = c21hip_h2d(d, p, bytes, stream);
    if (st) *status = st;
    return d;
}

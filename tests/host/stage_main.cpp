// The staging helpers' error path, without a device: built with hipcc together with csrc/pce_ctx.hip and run by tests/test_stage_host.py with no
// visible GPU.  An upload must come back as PCE_E_DEVICE, name THIS file and the call's line in pce_last_error, and leave the buffer empty.
#include <cstdio>
#include <cstring>
#include <vector>
#include "pce_internal.h"

static int upload(pce_ctx *c, DevBuf &b, const std::vector<float> &v, int *line)
{
    *line = __LINE__ + 1;
    PCE_UPLOAD(c, b, v, 64);
    return PCE_OK;
}

int main()
{
    pce_ctx c;
    DevBuf b;
    const std::vector<float> v(1000, 1.f);
    int line = 0;
    const int rc = upload(&c, b, v, &line);
    char want[64];
    snprintf(want, sizeof want, "stage_main.cpp:%d)", line);
    const char *err = pce_last_error(&c);
    printf("rc %d, error \"%s\", buffer {%p, %zu}\n", rc, err, b.p, b.cap);
    if (rc != PCE_E_DEVICE) { fprintf(stderr, "expected PCE_E_DEVICE (%d)\n", PCE_E_DEVICE); return 1; }
    if (!strstr(err, want)) { fprintf(stderr, "the error does not end in %s\n", want); return 1; }
    if (b.p != nullptr || b.cap != 0) { fprintf(stderr, "the buffer is not empty\n"); return 1; }
    return 0;
}

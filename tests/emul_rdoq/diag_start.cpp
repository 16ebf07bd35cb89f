// rdoq_diag_start of uvg266_amd/csrc/ctu_core.h -- the device RDOQ's closed form for the first scan index of a diagonal of the group
// grid -- compiled for the host and exported for tests/test_rdoq_diag_start.py, which builds this file itself (into pytest's
// temporary directory).  The host's own rdoq_wave walks group by group and does not use the function.
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include "ctu_core.h"

extern "C" __attribute__((visibility("default"))) int rdoq_diag_start_host(int n, int d) { return ctu::rdoq_diag_start(n, d); }

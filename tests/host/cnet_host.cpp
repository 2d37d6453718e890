// Host build of the convolutional network (csrc/cnet.hpp: the geometry of the packed
// weights, the pack step and one row evaluated from the packed weights -- the text the
// device kernel takes its layout from, compiled with g++) for tests/test_cnet_host.py:
// a shared library with C linkage that has oth_cnet_blob_bytes / oth_cnet_pack /
// oth_cnet_eval on host memory.  tests/host/cnet_san_main.cpp includes this file under
// -fsanitize=address,undefined.  Test infrastructure only.
#include <stdint.h>
#include <string.h>

#include "../../gymothelloenv_amd/csrc/cnet.hpp"

using namespace oth;

// 0 for arguments out of range
extern "C" uint64_t host_cnet_blob_bytes(int n, const CnetParams* p) {
    if (cnet_check(n, p)) return 0;
    return cnet_geo(n, *p).bytes();
}

// cnet_check's message into msg (at most cap bytes, "" where the arguments are in range)
extern "C" void host_cnet_check(int n, const CnetParams* p, char* msg, int cap) {
    const char* why = cnet_check(n, p);
    strncpy(msg, why ? why : "", (size_t)cap - 1);
    msg[cap - 1] = 0;
}

// the numbers of weights and biases the pack step reads (0 for params out of range)
extern "C" uint64_t host_cnet_weights(int n, const CnetParams* p) {
    return cnet_check(n, p) ? 0 : cnet_weights(cnet_geo(n, *p));
}
extern "C" uint64_t host_cnet_biases(int n, const CnetParams* p) {
    return cnet_check(n, p) ? 0 : cnet_biases(cnet_geo(n, *p));
}

// 0, 1 for params out of range, 2 for a bias out of range (blob: host_cnet_blob_bytes' bytes)
extern "C" int host_cnet_pack(int n, const CnetParams* p, const int8_t* w, const int32_t* b, uint8_t* blob) {
    if (cnet_check(n, p)) return 1;
    return cnet_pack(n, *p, w, b, blob) ? 2 : 0;
}

// 0, 1 for params out of range, 2 for a blob of another geometry or other shifts (nothing is written)
extern "C" int host_cnet_eval(int n, const CnetParams* p, int R, const uint8_t* blob, const uint64_t* boards,
                              const uint16_t* meta, const uint64_t* legal, int32_t* priors, int32_t* values,
                              int32_t* logits) {
    if (cnet_check(n, p)) return 1;
    const CnetGeo geo = cnet_geo(n, *p);
    for (int r = 0; r < R; ++r)
        if (!cnet_row(geo, blob, boards + (size_t)r * 2 * geo.W, meta[r], legal + (size_t)r * geo.W,
                      priors + (size_t)r * geo.nn, values + r, logits ? logits + (size_t)r * (geo.nn + 1) : nullptr))
            return 2;
    return 0;
}

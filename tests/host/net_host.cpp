// Host build of the network (csrc/net.hpp: the geometry of the packed weights, the
// pack step and one row's features, layers, head and integer softmax read from the
// packed weights -- the text the device kernel takes its layout and its per-element
// steps from, compiled with g++) for tests/test_net_host.py: a shared library with C
// linkage that has oth_net_blob_bytes / oth_net_pack / oth_net_eval on host memory.
// tests/host/net_san_main.cpp includes this file under -fsanitize=address,undefined.
// Test infrastructure only.
#include <stdint.h>

#include "../../gymothelloenv_amd/csrc/net.hpp"

using namespace oth;

extern "C" uint32_t host_net_exp2(int f) { return f >= 0 && f < 256 ? NET_EXP2[f] : 0u; }

// 0 for arguments out of range
extern "C" uint64_t host_net_blob_bytes(int n, const NetParams* p) {
    if (net_check(n, p)) return 0;
    return net_geo(n, *p).bytes();
}

// 0, 1 for params out of range, 2 for a bias out of range (blob: host_net_blob_bytes' bytes)
extern "C" int host_net_pack(int n, const NetParams* p, const int8_t* w, const int32_t* b, uint8_t* blob) {
    if (net_check(n, p)) return 1;
    return net_pack(n, *p, w, b, blob) ? 2 : 0;
}

// 0, 1 for params out of range, 2 for a blob of another geometry or other shifts (nothing is written)
extern "C" int host_net_eval(int n, const NetParams* p, int R, const uint8_t* blob, const uint64_t* boards,
                             const uint16_t* meta, const uint64_t* legal, int32_t* priors, int32_t* values,
                             int32_t* logits) {
    if (net_check(n, p)) return 1;
    const NetGeo geo = net_geo(n, *p);
    for (int r = 0; r < R; ++r)
        if (!net_row(geo, blob, boards + (size_t)r * 2 * geo.W, meta[r], legal + (size_t)r * geo.W,
                     priors + (size_t)r * geo.nn, values + r, logits ? logits + (size_t)r * (geo.nn + 1) : nullptr))
            return 2;
    return 0;
}

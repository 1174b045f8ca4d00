// The layout of the bounding-box tree (include/fgc.h: fgc_ray_tree_build), shared by its builder and the ray walk
// (fgc_raytree.hip) and by the closest-point walk (fgc_closest.hip): the constants of the format, where each part of the
// buffer starts.  Nothing here decides a byte of what is built; fgc_raytree.hip describes the format.
#pragma once
#include "fgc_raycast.h"

namespace fgc {

constexpr int RT_FAN = 8;                            // children per node
constexpr int RT_MAX_LEVELS = 10;                    // node levels of 2^30 faces
constexpr int RT_STACK = 7 * RT_MAX_LEVELS + 1;
constexpr int RT_NODE_F4 = RT_FAN * 6 / 4;           // a node as float4: 12
constexpr float RT_SLACK = 0x1p-21f;                 // 4 units in the last place, relative
constexpr float RT_TINY = 0x1p-125f;                 // ... and absolute, for a product that underflowed

struct RtShape {
    int depth, nleaf;
    int n[RT_MAX_LEVELS + 1];                // boxes of level L (n[0] = nleaf)
    unsigned noff[RT_MAX_LEVELS + 1];        // first node of level L (L >= 1) in the node array
};

struct RtLayout {
    RtShape s;
    int nrec;
    unsigned nodes;
    size_t face_of, boxes, total;            // byte offsets
};

static inline RtLayout rt_layout(int nf) {
    RtLayout l = {};
    l.nrec = cdiv(nf, RC_CHUNK) * RC_CHUNK;
    l.s.nleaf = l.s.n[0] = l.nrec / RC_CHUNK;
    int L = 0;
    unsigned off = 0;
    do {
        ++L;
        l.s.n[L] = cdiv(l.s.n[L - 1], RT_FAN);
        l.s.noff[L] = off;
        off += (unsigned)l.s.n[L];
    } while (l.s.n[L] > 1);
    l.s.depth = L;
    l.nodes = off;
    l.face_of = (size_t)l.nrec * 3 * sizeof(f32x4);
    l.boxes = l.face_of + (size_t)l.nrec * sizeof(int);          // (nrec is a multiple of 4: 16-byte aligned)
    l.total = l.boxes + (size_t)l.nodes * RT_NODE_F4 * sizeof(f32x4);
    return l;
}

}  // namespace fgc

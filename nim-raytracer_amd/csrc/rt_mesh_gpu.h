// rt_mesh_gpu.h — device passes of a mesh update (rt_scene_set_mesh_vertices):
// bounds and validation, face normals, the BVH refit and the binned faces.
// Every pointer is a device pointer, `stream` a hipStream_t; every function
// returns a hipError_t as int (0: ok).
#pragma once
#include <cstdint>

#include "rt_common.h"
#include "rt_frame.h"

namespace rtmi {

struct MeshBounds {
  double flo[3], fhi[3];  // bounds of the vertices the faces reference (the BVH margin's)
  double alo[3], ahi[3];  // calcAABB over every vertex, with the host loop's semantics
  int32_t nonfinite;      // a face references a NaN or infinite coordinate
};

// words of the scratch buffer rtmi_mesh_bounds needs (unsigned long long)
constexpr int kMeshBoundsWords = 32;

}  // namespace rtmi

extern "C" {
// Read-only pass over mesh arrays; waits for the stream and fills *out.
int rtmi_mesh_bounds(const double* v, int64_t nv, const int32_t* f, int64_t nf, unsigned long long* scratch,
                     rtmi::MeshBounds* out, void* stream);
// Face normals at n64 / n32 (the mesh's slice): calcNormals' operation
// sequence, or given != null: a copy of the caller's; n32 is (float) of n64.
int rtmi_mesh_normals(const double* v, const int32_t* f, const double* given, int64_t nf, double* n64, float* n32,
                      void* stream);
// Refit of the nodes [node0, node0 + nnode) of one mesh, bottom-up: leaf
// children from their faces (order: leaf slot -> face; a leaf child's c is
// tri_base + its first slot), inner children from that node's two boxes. The
// same boxes go into nodes64 and nodes32 (both indexed by node; the child
// references differ and are not touched). parent[node]: 2 * parent + slot, -1
// for a root. arrivals: nnode zeroed counters at arrivals[node - node0].
int rtmi_mesh_refit(const double* v, const int32_t* f, const int32_t* order, double inflate, int32_t node0,
                    int32_t nnode, int64_t tri_base, const int32_t* parent, int32_t* arrivals,
                    rtmi::BvhNode* nodes64, rtmi::BvhNode* nodes32, void* stream);
// The binned faces in leaf order: vertices, rec = rec0 + 64 * slot, face.
int rtmi_mesh_bins(const double* v, const int32_t* f, const int32_t* order, int64_t nf, int64_t rec0,
                   rtmi::DevBinTri* out, void* stream);
}

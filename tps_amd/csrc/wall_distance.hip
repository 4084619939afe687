// The wall-distance function of libtpsrhs.so (wall_faces.hpp, wall_distance.hpp): tpsrhs_wall_faces and
// tpsrhs_wall_distance.  No operator state: the face table lives on the device for the length of one call.
#include "abi_support.hpp"
#include "wall_distance.hpp"
#include "wall_faces.hpp"

#include <cmath>

namespace {
template <int DIM>
void launch_wall_distance(tpsrhs_operator *h, int64_t nfaces, const double *face_xyz, double *out) {
  std::vector<double> coef;
  wd_face_table<DIM>(nfaces, face_xyz, coef);
  WdNodes nodes = {};
  double wts[TPSRHS_MAXORDER + 1];
  segment_rule01(h->nc, h->order + 1, nodes.x, wts);  // the nodes of the operator's basis, as make_tables places them
  const int64_t grid = (h->ndofs + WD_BLOCK - 1) / WD_BLOCK;
  if (grid == 0) return;
  if (grid >= (int64_t(1) << 31)) throw Unsupported("tpsrhs_wall_distance: more than 2^39 nodes");
  const char *env = std::getenv("TPSRHS_WALLDIST_CULL");
  const bool cull = !(env && env[0] == '0');
  const DevBuf<double> table(coef);
  const dim3 g(static_cast<unsigned>(grid)), b(WD_BLOCK);
  if (cull)
    hipLaunchKernelGGL((k_wall_distance<DIM, true>), g, b, 0, h->stream, h->ndofs, h->order + 1, nodes, h->d_verts.get(), nfaces,
                       table.get(), out);
  else
    hipLaunchKernelGGL((k_wall_distance<DIM, false>), g, b, 0, h->stream, h->ndofs, h->order + 1, nodes, h->d_verts.get(), nfaces,
                       table.get(), out);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(h->stream));  // the table is freed on return
}
}  // namespace

extern "C" {

int tpsrhs_wall_faces(const tpsrhs_mesh *mesh, int num_bcs, const tpsrhs_bc *bcs, int num_attributes, const int *attributes,
                      int64_t capacity, double *face_xyz_out, int64_t *num_faces_out) {
  const int st = wall_faces(mesh, num_bcs, bcs, num_attributes, attributes, capacity, face_xyz_out, num_faces_out);
  if (st != TPSRHS_OK)
    return fail(st, "tpsrhs_wall_faces: needs a mesh of dim 2 or 3 whose boundary records are faces of its elements, the attribute list or the boundary conditions, capacity >= 0 with its array, and num_faces_out");
  return st;
}

int tpsrhs_patch_faces(const tpsrhs_mesh *mesh, int num_attributes, const int *attributes, int64_t capacity, int32_t *elem_out,
                       int32_t *face_out, int32_t *patch_out, int64_t *num_faces_out) {
  const int st = patch_faces(mesh, num_attributes, attributes, capacity, elem_out, face_out, patch_out, num_faces_out);
  if (st != TPSRHS_OK)
    return fail(st, "tpsrhs_patch_faces: needs a mesh of dim 2 or 3 whose boundary records are faces of its elements, num_attributes >= 1 distinct attributes, capacity >= 0 with its arrays, and num_faces_out");
  return st;
}

int tpsrhs_wall_distance(tpsrhs_handle h, int64_t num_faces, const double *face_xyz, double *distance_out) {
  if (!h || !distance_out || num_faces < 0 || (num_faces > 0 && !face_xyz))
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_wall_distance: needs a handle, num_faces >= 0, the faces and the output array");
  const int64_t nval = num_faces * (int64_t(1) << (h->dim - 1)) * h->dim;
  for (int64_t i = 0; i < nval; i++)
    if (!std::isfinite(face_xyz[i]))
      return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_wall_distance: face coordinate " + std::to_string(i) + " is not finite");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    if (h->dim == 3)
      launch_wall_distance<3>(h, num_faces, face_xyz, distance_out);
    else
      launch_wall_distance<2>(h, num_faces, face_xyz, distance_out);
  });
}

}  // extern "C"

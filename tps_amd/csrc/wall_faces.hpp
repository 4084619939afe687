// Which boundary faces are walls, and where their corners are: the host half of the wall-distance function
// (tpsrhs_wall_faces; the device half is wall_distance.hpp) -- and which (element, local face) pairs make a boundary patch:
// the host half of the surface integrals (tpsrhs_patch_faces; the device half is surface.hpp).  The reference selects the
// wall faces inside its node loop, by comparing every boundary element's attribute with the wall patches
// (src/utils.cpp:403-412), and collects the patches from its boundary conditions: every wall that is not inviscid
// (src/M2ulPhyS.cpp:392-398).
// Plain C++: no HIP, no device, nothing but tpsrhs.h -- a stand-alone program can include this file alone
// (tests/test_wall_faces_sanitize.py does, under the sanitizers).
//
// A boundary record of tpsrhs_mesh names its face by topological vertex ids, in an order that is NOT cyclic for
// hexahedron faces; the corners therefore come from the owning element's local face (face_corners in topology.hpp: local
// face f = 2 d + s is xi_d = s, its tangential axes (a, b) the remaining axes in increasing order), corner = ta + 2 tb,
// with the coordinates of the element's own elem_coords: periodic meshes keep their geometry.
#ifndef TPSRHS_WALL_FACES_HPP_
#define TPSRHS_WALL_FACES_HPP_

#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/tpsrhs.h"

namespace tpsrhs {

// MFEM corner v of a quadrilateral / hexahedron -> lexicographic corner (bit d = reference coordinate d)
inline int wall_lex_corner(int v) {
  static const int quad[4] = {0, 1, 3, 2};
  return (v & 4) | quad[v & 3];
}

// lexicographic corners of local face f in (ta, tb) order: topology.hpp::face_corners, restated so that this header
// stands alone
inline void wall_face_corners(int dim, int f, int *c) {
  const int d = f >> 1, s = f & 1;
  if (dim == 2) {
    const int a = 1 - d;
    for (int ta = 0; ta < 2; ta++) c[ta] = (s << d) | (ta << a);
  } else {
    const int a = (d == 0) ? 1 : 0, b = (d == 2) ? 1 : 2;
    for (int tb = 0; tb < 2; tb++)
      for (int ta = 0; ta < 2; ta++) c[ta + 2 * tb] = (s << d) | (ta << a) | (tb << b);
  }
}

// The boundary records of a mesh matched to the element faces that carry them: visit(e, f, b, c, mfem_of_lex) for every
// record b, in ascending (element, local face) order of its owner; c: the lexicographic corners of local face f
// (wall_face_corners), mfem_of_lex: the element's corner numbering.  A record is taken by the FIRST element face that carries
// its vertices (on a periodic mesh an "interior boundary" has two).  TPSRHS_ERR_INVALID_ARGUMENT after the visits if a
// record is no element's face.  The caller has checked the mesh's arrays.
template <class F>
inline int for_each_boundary_face(const tpsrhs_mesh *mesh, F &&visit) {
  const int ne = mesh->num_elements, nb = mesh->num_bdr_faces;
  const int dim = mesh->dim, nvpe = 1 << dim, nfv = 1 << (dim - 1), nlf = 2 * dim;
  // the boundary records by their sorted vertex ids
  typedef std::array<int, 4> Key;
  auto make_key = [&](const int *ids) {
    Key k = {-1, -1, -1, -1};
    for (int i = 0; i < nfv; i++) k[i] = ids[i];
    std::sort(k.begin(), k.begin() + nfv);
    return k;
  };
  std::vector<std::pair<Key, int>> recs(static_cast<size_t>(nb));
  for (int b = 0; b < nb; b++) recs[static_cast<size_t>(b)] = {make_key(mesh->bdr_vertices + static_cast<size_t>(b) * nfv), b};
  std::sort(recs.begin(), recs.end());
  std::vector<char> matched(static_cast<size_t>(nb), 0);
  for (int e = 0; e < ne; e++) {
    const int *ev = mesh->elem_vertices + static_cast<size_t>(e) * nvpe;
    int mfem_of_lex[8];
    for (int v = 0; v < nvpe; v++) mfem_of_lex[wall_lex_corner(v)] = v;
    for (int f = 0; f < nlf; f++) {
      int c[4], ids[4];
      wall_face_corners(dim, f, c);
      for (int i = 0; i < nfv; i++) ids[i] = ev[mfem_of_lex[c[i]]];
      const Key key = make_key(ids);
      auto it = std::lower_bound(recs.begin(), recs.end(), std::make_pair(key, -1));
      for (; it != recs.end() && it->first == key; ++it) {
        const int b = it->second;
        if (matched[static_cast<size_t>(b)]) continue;
        matched[static_cast<size_t>(b)] = 1;
        visit(e, f, b, c, mfem_of_lex);
      }
    }
  }
  for (int b = 0; b < nb; b++)
    if (!matched[static_cast<size_t>(b)]) return TPSRHS_ERR_INVALID_ARGUMENT;  // a boundary record that is no element's face
  return TPSRHS_OK;
}

// tpsrhs_wall_faces without the error text: a tpsrhs_status
inline int wall_faces(const tpsrhs_mesh *mesh, int num_bcs, const tpsrhs_bc *bcs, int num_attributes, const int *attributes,
                      int64_t capacity, double *face_xyz_out, int64_t *num_faces_out) {
  if (num_faces_out) *num_faces_out = 0;
  if (!mesh || !num_faces_out || capacity < 0 || (capacity > 0 && !face_xyz_out)) return TPSRHS_ERR_INVALID_ARGUMENT;
  if (mesh->dim != 2 && mesh->dim != 3) return TPSRHS_ERR_INVALID_ARGUMENT;
  if (num_attributes > 0 && !attributes) return TPSRHS_ERR_INVALID_ARGUMENT;
  if (num_attributes < 0 && (num_bcs < 0 || (num_bcs > 0 && !bcs))) return TPSRHS_ERR_INVALID_ARGUMENT;
  const int ne = mesh->num_elements, nb = mesh->num_bdr_faces;
  if (ne < 0 || nb < 0 || (ne > 0 && (!mesh->elem_vertices || !mesh->elem_coords))) return TPSRHS_ERR_INVALID_ARGUMENT;
  if (nb > 0 && (!mesh->bdr_vertices || !mesh->bdr_attributes)) return TPSRHS_ERR_INVALID_ARGUMENT;
  const int dim = mesh->dim, nvpe = 1 << dim, nfv = 1 << (dim - 1);

  std::vector<int> wall;  // the selected attributes
  if (num_attributes >= 0) {
    wall.assign(attributes, attributes + num_attributes);
  } else {
    for (int k = 0; k < num_bcs; k++)
      if (bcs[k].category == TPSRHS_WALL && bcs[k].type != TPSRHS_INV) wall.push_back(bcs[k].attribute);
  }
  auto is_wall = [&](int attr) { return std::find(wall.begin(), wall.end(), attr) != wall.end(); };

  int64_t count = 0;
  const int st = for_each_boundary_face(mesh, [&](int e, int f, int b, const int *c, const int *mfem_of_lex) {
    (void)f;
    if (!is_wall(mesh->bdr_attributes[b])) return;
    const double *ex = mesh->elem_coords + static_cast<size_t>(e) * nvpe * dim;
    if (count < capacity)
      for (int i = 0; i < nfv; i++)
        for (int d = 0; d < dim; d++)
          face_xyz_out[(static_cast<size_t>(count) * nfv + i) * dim + d] = ex[mfem_of_lex[c[i]] * dim + d];
    count++;
  });
  *num_faces_out = count;
  return st;
}

// tpsrhs_patch_faces without the error text: a tpsrhs_status.  The boundary faces whose attribute is attributes[p], as
// (element, local face, p), in ascending (element, local face) order; what BoundaryCondition::aggregateBndryFaces
// (src/BoundaryCondition.cpp:76-92) counts per patch, with the faces themselves.
inline int patch_faces(const tpsrhs_mesh *mesh, int num_attributes, const int *attributes, int64_t capacity, int32_t *elem_out,
                       int32_t *face_out, int32_t *patch_out, int64_t *num_faces_out) {
  if (num_faces_out) *num_faces_out = 0;
  if (!mesh || !num_faces_out || capacity < 0 || (capacity > 0 && (!elem_out || !face_out || !patch_out)))
    return TPSRHS_ERR_INVALID_ARGUMENT;
  if (mesh->dim != 2 && mesh->dim != 3) return TPSRHS_ERR_INVALID_ARGUMENT;
  if (num_attributes < 1 || !attributes) return TPSRHS_ERR_INVALID_ARGUMENT;
  for (int p = 0; p < num_attributes; p++)
    if (std::find(attributes, attributes + p, attributes[p]) != attributes + p) return TPSRHS_ERR_INVALID_ARGUMENT;
  const int ne = mesh->num_elements, nb = mesh->num_bdr_faces;
  if (ne < 0 || nb < 0 || (ne > 0 && !mesh->elem_vertices)) return TPSRHS_ERR_INVALID_ARGUMENT;
  if (nb > 0 && (!mesh->bdr_vertices || !mesh->bdr_attributes)) return TPSRHS_ERR_INVALID_ARGUMENT;
  int64_t count = 0;
  const int st = for_each_boundary_face(mesh, [&](int e, int f, int b, const int *, const int *) {
    const int *at = std::find(attributes, attributes + num_attributes, mesh->bdr_attributes[b]);
    if (at == attributes + num_attributes) return;
    if (count < capacity) {
      elem_out[count] = e;
      face_out[count] = f;
      patch_out[count] = static_cast<int32_t>(at - attributes);
    }
    count++;
  });
  *num_faces_out = count;
  return st;
}

}  // namespace tpsrhs
#endif

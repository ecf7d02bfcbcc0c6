// The per-face forward of the mesh binding (mpmavatar_amd/csrc/frames_math.hpp) compiled for the host (tests/test_frames_host.py; the
// stand-in for <hip/hip_runtime.h> is tests/hostmath/stub): the serial loop over frm::face_frame_row that mirrors k_face_frames.
#include "frames_math.hpp"

#include <cstdint>

extern "C" void hfr_face_frames(const float *verts, const int32_t *faces, int n_f, float *center, float *mat, float *quat, float *scale) {
  for (int f = 0; f < n_f; ++f) frm::face_frame_row(f, verts, faces, center, mat, quat, scale);
}

// The matrix -> quaternion map as the BACKWARD states it (quat_branch, quat_numerators, norm4) on a saved face_orien_mat [n_f, 3, 3]:
// the branch [n_f] and the unit quaternion WXYZ [n_f, 4], which must be the forward's bits.
extern "C" void hfr_quat_from_pieces(const float *mat, int n_f, int32_t *branch, float *quat) {
  for (int f = 0; f < n_f; ++f) {
    float R[3][3], q[4];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) R[r][c] = mat[9 * (int64_t)f + 3 * r + c];
    branch[f] = frm::quat_branch(R);
    frm::quat_numerators(R, branch[f], q);
    const float n = frm::norm4(q);
    float *o = quat + 4 * (int64_t)f;
    o[0] = q[3] / n; o[1] = q[0] / n; o[2] = q[1] / n; o[3] = q[2] / n;
  }
}

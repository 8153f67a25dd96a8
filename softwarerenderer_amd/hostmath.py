"""Host-side input generators: the System.Numerics.Matrix4x4 factories the C# host uses to
build the matrices it passes to RenderMesh (Renderer.cs:406-410, Camera.cs:12-17).  They only
MAKE inputs (float32, row-major M11..M44, row-vector convention); the hot path never calls them."""
from __future__ import annotations

import numpy as np

F = np.float32


def identity() -> np.ndarray:
    return np.eye(4, dtype=F)


def create_scale(s) -> np.ndarray:
    m = np.eye(4, dtype=F)
    m[0, 0] = m[1, 1] = m[2, 2] = F(s)
    return m


def create_translation(x, y, z) -> np.ndarray:
    m = np.eye(4, dtype=F)
    m[3, 0], m[3, 1], m[3, 2] = F(x), F(y), F(z)
    return m


def create_rotation_y(rad) -> np.ndarray:
    c, s = F(np.cos(F(rad))), F(np.sin(F(rad)))
    m = np.eye(4, dtype=F)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = c, -s, s, c
    return m


def create_rotation_x(rad) -> np.ndarray:
    c, s = F(np.cos(F(rad))), F(np.sin(F(rad)))
    m = np.eye(4, dtype=F)
    m[1, 1], m[1, 2], m[2, 1], m[2, 2] = c, s, -s, c
    return m


def create_perspective_fov(fov_rad, aspect, near, far) -> np.ndarray:
    """Matrix4x4.CreatePerspectiveFieldOfView (right-handed, z in [0,1])."""
    y_scale = F(1.0) / F(np.tan(F(fov_rad) * F(0.5)))
    x_scale = y_scale / F(aspect)
    m = np.zeros((4, 4), dtype=F)
    m[0, 0] = x_scale
    m[1, 1] = y_scale
    neg_far_range = F(-1.0) if np.isposinf(far) else F(far) / (F(near) - F(far))
    m[2, 2] = neg_far_range
    m[2, 3] = F(-1.0)
    m[3, 2] = F(near) * neg_far_range
    return m


def create_look_at(eye, target, up) -> np.ndarray:
    """Matrix4x4.CreateLookAt (right-handed)."""
    eye, target, up = (np.asarray(a, dtype=F) for a in (eye, target, up))
    z = eye - target
    z = z / F(np.sqrt(F(z @ z)))
    x = np.cross(up, z).astype(F)
    x = x / F(np.sqrt(F(x @ x)))
    y = np.cross(z, x).astype(F)
    m = np.eye(4, dtype=F)
    m[0, 0], m[1, 0], m[2, 0] = x
    m[0, 1], m[1, 1], m[2, 1] = y
    m[0, 2], m[1, 2], m[2, 2] = z
    m[3, 0], m[3, 1], m[3, 2] = -F(x @ eye), -F(y @ eye), -F(z @ eye)
    return m


# the cameras of a cube map's six faces (+X, -X, +Y, -Y, +Z, -Z): where each looks and what it holds up (swr_cube_face_view)
CUBE_FACE_AXIS = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))
CUBE_FACE_UP = ((0, 1, 0), (0, 1, 0), (0, 0, 1), (0, 0, -1), (0, 1, 0), (0, 1, 0))
_CUBE_X = ((0, 0, 1), (0, 0, -1), (1, 0, 0), (1, 0, 0), (-1, 0, 0), (1, 0, 0))
_CUBE_Y = ((0, 1, 0), (0, 1, 0), (0, 0, 1), (0, 0, -1), (0, 1, 0), (0, 1, 0))
_CUBE_Z = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


def cube_face_view(face: int, eye) -> np.ndarray:
    """create_look_at(eye, eye + CUBE_FACE_AXIS[face], CUBE_FACE_UP[face]) with the camera's axes taken as the exact unit vectors
    they are (eye + axis - eye is not the axis for every float eye).  Under create_perspective_fov(pi / 2, 1, near, far) the pixel
    whose centre lies in direction d from eye is the texel texture_cube_face(d) names."""
    if not 0 <= int(face) <= 5:
        raise ValueError("face must be 0 .. 5 (+X, -X, +Y, -Y, +Z, -Z)")
    eye = np.asarray(eye, dtype=F)
    m = np.eye(4, dtype=F)
    for k, table in enumerate((_CUBE_X, _CUBE_Y, _CUBE_Z)):
        a = np.asarray(table[int(face)], dtype=F)
        m[0, k], m[1, k], m[2, k] = a
        m[3, k] = -F(F(F(a[0] * eye[0]) + F(a[1] * eye[1])) + F(a[2] * eye[2]))
    return m


def multiply(a, b) -> np.ndarray:
    return (np.asarray(a, dtype=F) @ np.asarray(b, dtype=F)).astype(F)


def invert(m):
    """Matrix4x4.Invert for the normal matrix of Physics.Raycast (Physics.cs:30-38): the inverse, or None where the reference's
    `if (!Matrix4x4.Invert(...)) return false` applies.  BUILD-DEFINED: the inverse is computed in float64 and rounded to float32,
    and None is returned when the float64 determinant is 0 or not finite; the numerics of .NET's own Invert are pinned by nothing,
    which is why swr_ray_target takes the caller's matrix."""
    a = np.asarray(m, dtype=F).reshape(4, 4).astype(np.float64)
    with np.errstate(all="ignore"):
        det = np.linalg.det(a)
        if det == 0.0 or not np.isfinite(det):
            return None
        try:
            inv = np.linalg.inv(a)
        except np.linalg.LinAlgError:
            return None
    return inv.astype(F)


def normal_matrix(model):
    """Transpose(Invert(model)) as Physics.Raycast forms it (Physics.cs:38), or None where the model does not invert."""
    inv = invert(model)
    return None if inv is None else np.ascontiguousarray(inv.T)


def create_from_quaternion(q) -> np.ndarray:
    """Matrix4x4.CreateFromQuaternion (q = x, y, z, w), in that source's term order, float32 with one rounding per operation: the
    rotation block of a skeleton node's local matrix (include/swr.h "SKELETAL ANIMATION")."""
    x, y, z, w = (F(v) for v in np.asarray(q, dtype=F).reshape(4))
    one, two = F(1.0), F(2.0)
    with np.errstate(all="ignore"):
        xx, yy, zz = x * x, y * y, z * z
        xy, wz, xz, wy, yz, wx = x * y, z * w, z * x, y * w, y * z, x * w
        m = np.eye(4, dtype=F)
        m[0, 0], m[0, 1], m[0, 2] = one - two * (yy + zz), two * (xy + wz), two * (xz - wy)
        m[1, 0], m[1, 1], m[1, 2] = two * (xy - wz), one - two * (zz + xx), two * (yz + wx)
        m[2, 0], m[2, 1], m[2, 2] = two * (xz + wy), two * (yz - wx), one - two * (yy + xx)
    return m


def quaternion_lerp(a, b, u) -> np.ndarray:
    """Quaternion.Lerp(a, b, u) in its scalar form: the normalised lerp along the shorter arc (not a slerp); u is not clamped and a
    zero result gives the NaN it gives."""
    a, b, u = np.asarray(a, dtype=F).reshape(4), np.asarray(b, dtype=F).reshape(4), F(u)
    with np.errstate(all="ignore"):
        u1 = F(1.0) - u
        dot = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]
        r = np.array([u1 * a[c] + u * b[c] if dot >= 0 else u1 * a[c] - u * b[c] for c in range(4)], dtype=F)
        ls = ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]
        inv = F(1.0) / np.sqrt(ls)
        return (r * inv).astype(F)

"""Child of tests/test_gpu_post.py (started through tests/spawner.py, never imported by pytest): runs one post program under the library
that SWR_LIB names, on a frame read from a file, and writes the float payload to another.

    post_child.py PROGRAM KX KY FRAME.npy CONSTANTS.npy OUT.npy
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import post_cases as P                                                 # noqa: E402
from softwarerenderer_amd import Device, MainWindow, PostProgram      # noqa: E402


def main(program, kx, ky, frame_path, constants_path, out_path):
    color = np.load(frame_path)
    dev = Device(0)
    fma, _ = dev.numerics_mode()
    win = MainWindow(dev, color.shape[1], color.shape[0])
    win.Upload(color=color)
    post = PostProgram(dev, getattr(P, program), constants=np.load(constants_path))
    out = win.PostBuffer(post, kx, ky, 3, np.float32)
    post.close()
    np.save(out_path, out)
    print(f"library={os.path.basename(os.environ.get('SWR_LIB', '') or 'libswr_hip.so')} lerp_fused={int(bool(fma))}")
    dev.close()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5], sys.argv[6])

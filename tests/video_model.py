"""TEST INFRASTRUCTURE ONLY - the numpy statement of the video path's two operators (include/unet_hip.h:
unet_resize_u8_batch, unet_overlay_u8_batch).  The kernels are checked against it bit for bit.

The resize is oracle/camera_oracle.resize_linear (cv::resize INTER_LINEAR, 8-bit, restated; equal sizes are a copy).
The blend is cv2.addWeighted in fp32: every product and every sum is rounded to float32 on its own - numpy has no fused
multiply-add - and the result is rounded half to even (np.rint) and saturated.  Parity against cv2 itself is unpinned.
"""
import numpy as np

from oracle.camera_oracle import resize_linear


def resize_batch(src, out_w, out_h, swap_rb=False):
    """(N,H,W) or (N,H,W,C) uint8 -> (N,out_h,out_w[,C]); with swap_rb channels 0 and 2 are exchanged."""
    src = np.asarray(src)
    out = np.stack([resize_linear(img, out_w, out_h) for img in src])
    return np.ascontiguousarray(out[..., ::-1]) if swap_rb else out


def blend(frame, colour, alpha, beta, gamma):
    """addWeighted on uint8 arrays of one shape: clamp(rint(fl(fl(fl(frame*alpha) + fl(colour*beta)) + gamma)))"""
    f32 = np.float32
    a = (frame.astype(f32) * f32(alpha)).astype(f32)
    b = (colour.astype(f32) * f32(beta)).astype(f32)
    v = ((a + b).astype(f32) + f32(gamma)).astype(f32)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def overlay_batch(frames, masks, lut, alpha, beta, gamma):
    """frames (N,H,W,3), masks (N,h,w), lut (256,3) uint8 -> (overlay (N,H,W,3), mask (N,H,W))"""
    frames, lut = np.asarray(frames), np.asarray(lut)
    h, w = frames.shape[1:3]
    m = resize_batch(masks, w, h)
    return blend(frames, lut[m], alpha, beta, gamma), m

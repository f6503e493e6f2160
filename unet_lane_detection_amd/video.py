"""The reference's video mode on the GPU, a chunk of frames at a time.

Reference: `RKNNLaneInference.predict_video` (src/unet.py:99-140), which `src/unet.py`'s `__main__` runs; the webcam
and single-image modes (:190-224, :242-257) do the same three things per frame:
    predict(cvtColor(frame, BGR2RGB))                      resize to 224x224, network, > threshold, * 255, resize back
    lane_colored = cv2.applyColorMap(mask, COLORMAP_JET)
    result = cv2.addWeighted(frame, 0.7, lane_colored, 0.3, 0)
Here a chunk of BGR frames is resized with the colour swap in one launch (`unet_resize_u8_batch`), goes through the
network (`run_u8`), and the small masks come back as overlay and full-size mask in one pass over the frames
(`unet_overlay_u8_batch`; tests/video_model.py states the arithmetic).  `FramePipeline.run` keeps the device busy while
chunks cross PCIe.  Decoding and encoding stay with the caller.  No CPU fallback.

UNPINNED: OpenCV (cv2) is not installed and the reference holds no fixture for this stage, so neither the resize (see
oracle/camera_oracle.py) nor the colour map is compared with cv2 itself.
"""
from __future__ import annotations

import ctypes as C
import inspect
import time

import numpy as np
import torch

from . import _lib


def jet_table():
    """The default colour map: (256, 3) uint8 in B, G, R order, the classic jet ramp stated in integers so that no
    implementation can disagree on a tie:
        lut[i][k] = (clamp(765 - 2 * |4 i - 255 c_k|, 0, 510) + 1) // 2,   c = (1, 2, 3) for (B, G, R).
    Entry 0 is (128, 0, 0), entry 255 is (0, 0, 128).  UNPINNED against cv2.COLORMAP_JET: OpenCV builds its table from
    stored samples and cv2 is not installed here; a user who has cv2 can pass its table as `lut`."""
    i = np.arange(256, dtype=np.int64)[:, None]
    c = np.array([1, 2, 3], dtype=np.int64)[None, :]
    return ((np.clip(765 - 2 * np.abs(4 * i - 255 * c), 0, 510) + 1) // 2).astype(np.uint8)


def check_mask_class(model, mask_class):
    """The argument checks of a pipeline that takes a model's mask: a K-class model (out_channels > 1) needs the class
    whose byte plane it is to use, a single-class model takes none.  Returns mask_class as an int, or None."""
    k = int(getattr(model, "out_channels", 1))
    if k > 1:
        if mask_class is None:
            raise ValueError(f"the model has {k} classes: mask_class names the one whose pixels are the mask")
        if not 0 <= int(mask_class) < k:
            raise ValueError(f"mask_class={mask_class!r}: the model has classes 0..{k - 1}")
        return int(mask_class)
    if mask_class is not None:
        raise ValueError("mask_class belongs to a K-class model (out_channels > 1)")
    return None


class FramePipeline:
    """BGR frames -> (overlay, mask) through a `UNetHIP` (on the tier `precision`) or a `UNetInt8`.

    diagnose=True: every chunk is also measured where it already is, before the resize
    (diagnose.frame_records: pixel range, brightness, Laplacian sharpness per frame), and `process` and `run` hand out
    ((overlay, mask), diagnose.FrameStats) instead of (overlay, mask).  Overlay and mask are the same either way.

    correct=correct.CorrectConfig(...): every chunk's BGR frames are corrected on the device before the resize
    (correct.FrameCorrector, into a buffer of the pipeline's own): the network sees and the overlay is blended onto
    the corrected frames, while `diagnose` still measures the frames as they came.  correct=None: every launch, every
    buffer and every return value as without it."""

    SLOTS = 3   # chunk k computes while k+1 is uploaded and k-1 is downloaded

    def __init__(self, model, threshold=0.5, input_size=(224, 224), precision="f16x3", lut=None, alpha=0.7, beta=0.3,
                 gamma=0.0, diagnose=False, correct=None, mask_class=None):
        """input_size: (width, height) of the network's input; lut: (256, 3) uint8 in the frames' channel order
        (default `jet_table()`); alpha, beta, gamma: cv2.addWeighted's.  mask_class: the class of a K-class model
        (out_channels > 1) whose pixels are the mask - required for such a model, refused for a single-class one, whose
        mask is `threshold`'s."""
        self.mask_class = check_mask_class(model, mask_class)
        if not torch.cuda.is_available():
            raise RuntimeError("FramePipeline needs a HIP device; there is no CPU fallback")
        self._lib = _lib.load()
        self.model = model
        self.device = model.device
        self.threshold = threshold
        self.input_size = (int(input_size[0]), int(input_size[1]))
        # UNetInt8.run_u8 has one arithmetic and no `precision` argument
        self._tiered = "precision" in inspect.signature(model.run_u8).parameters
        self.precision = precision if self._tiered else None
        lut = jet_table() if lut is None else np.ascontiguousarray(lut, dtype=np.uint8)
        if lut.shape != (256, 3):
            raise ValueError("lut must be (256, 3) uint8")
        self.lut = lut
        self.alpha, self.beta, self.gamma = float(alpha), float(beta), float(gamma)
        self._streams = None
        self.diagnose = bool(diagnose)
        self.correct = correct
        self.corrector = self._corrected = None
        if correct is not None:
            from .correct import FrameCorrector
            self.corrector = FrameCorrector(correct, device=self.device)

    # ---- the three stages, each on torch's current stream -----------------------------------------------------
    def _resize(self, frames):
        n, h, w, _ = frames.shape
        in_w, in_h = self.input_size
        small = torch.empty((n, in_h, in_w, 3), dtype=torch.uint8, device=self.device)
        _lib.call("unet_resize_u8_batch", self.device, frames, n, h, w, 3, 1, in_w, in_h, small)
        return small

    def _network(self, small):
        if self.mask_class is not None:   # a K-class model: the byte plane of one class stands where the thresholded mask stands
            kw = {"precision": self.precision} if self._tiered else {}
            return self.model.run_u8(small, mask_class=self.mask_class, **kw)[-1]
        if not self._tiered:
            return self.model.run_u8(small, return_mask=True, threshold=self.threshold)[-1]
        return self.model.run_u8(small, return_mask=True, threshold=self.threshold, precision=self.precision)[-1]

    def _verify(self):
        """The device's verdict on the forwards launched since the last call (synchronises the current stream), as
        `LanePipelineGPU._run_checked`: a kernel-side failure raises; after a range report of the f16x3 tier the
        pipeline moves to the exact-fp32 tier for good and False tells the caller to run the chunk again."""
        if not self._tiered:
            return True
        rc = self.model.device_error(current_stream_only=True)
        if rc == 0:
            return True
        if rc == _lib.UNET_ERR_RANGE and self.precision == "f16x3":
            print("unet_hip: an activation left the fp16 range of the f16x3 tier; continuing on the fp32 tier")
            self.precision = "fp32"
            return False
        raise _lib.UnetError(rc, "unet_device_error")

    def _overlay(self, frames, mask_small, overlay, mask):
        n, h, w, _ = frames.shape
        _lib.call("unet_overlay_u8_batch", self.device, frames, n, h, w, mask_small, int(mask_small.shape[1]),
                  int(mask_small.shape[2]), self.lut.ctypes.data_as(C.c_void_p), self.alpha, self.beta, self.gamma, overlay,
                  mask)

    def _launch(self, frames, overlay, mask):
        if self.corrector is not None:
            # the buffer only grows, and every use of it is enqueued on one stream after the other
            if self._corrected is None or self._corrected.numel() < frames.numel():
                if self._corrected is not None:
                    self._corrected.record_stream(torch.cuda.current_stream(self.device))
                self._corrected = torch.empty(frames.numel(), dtype=torch.uint8, device=self.device)
            frames = self.corrector.correct(frames, bgr=True, out=self._corrected[:frames.numel()].view(frames.shape))
        self._overlay(frames, self._network(self._resize(frames)), overlay, mask)

    def _measure(self, frames):
        """diagnose: the chunk's records, enqueued on the current stream and left on the device"""
        from .diagnose import frame_records
        n, h, w, _ = frames.shape
        return frame_records(frames, n, h, w, 0, True)

    @staticmethod
    def _frame_stats(records, shape):
        from .diagnose import FRAME_WORDS, FrameStats
        words = records.cpu().numpy().view(np.uint64).reshape(shape[0], FRAME_WORDS)
        return FrameStats(words, shape[1], shape[2])

    def process(self, frames_bgr):
        """(N,H,W,3) uint8 BGR, numpy or torch, host or device -> (overlay (N,H,W,3), mask (N,H,W)) device tensors;
        `mask` is what the reference's `predict` returns for each frame.  With `diagnose`: ((overlay, mask),
        FrameStats of the chunk)."""
        frames = torch.as_tensor(frames_bgr)
        if frames.dim() != 4 or frames.shape[-1] != 3 or frames.dtype != torch.uint8:
            raise ValueError("frames must be (N,H,W,3) uint8")
        frames = frames.to(self.device).contiguous()
        overlay = torch.empty_like(frames)
        mask = torch.empty(frames.shape[:3], dtype=torch.uint8, device=self.device)
        records = self._measure(frames) if self.diagnose else None
        self._launch(frames, overlay, mask)
        if not self._verify():
            self._launch(frames, overlay, mask)
            self._verify()
        if self.diagnose:
            return (overlay, mask), self._frame_stats(records, frames.shape)
        return overlay, mask

    # ---- streamed chunks ---------------------------------------------------------------------------------------
    def run(self, chunks):
        """chunks: an iterable of (N,H,W,3) uint8 BGR host arrays (N and the frame size may change from chunk to
        chunk).  Yields (overlay, mask) as host numpy arrays, in order; what is yielded is fresh memory that no later
        chunk overwrites - the two arrays of a chunk are views of one page-locked block of their own, which goes back to
        torch's host allocator when both are dropped, so a caller who keeps many chunks should copy them.  Pinned
        staging buffers and three streams (copy in, compute, copy out) tied by events: chunk
        k+1 is uploaded and chunk k-1 is downloaded while chunk k computes, and the host's own copies (into and out of
        the staging buffers) are done in that time too: the device's verdict on chunk k is awaited after them.  No
        thread and no process is created.  With `diagnose` every item is ((overlay, mask), FrameStats of the chunk)."""
        if self._streams is None:
            self._streams = tuple(torch.cuda.Stream(self.device) for _ in range(3))
        s_in, s_run, s_out = self._streams
        slots = [dict(cap=-1) for _ in range(self.SLOTS)]

        def upload(k, chunk):
            a = np.ascontiguousarray(chunk)
            if a.ndim != 4 or a.shape[-1] != 3 or a.dtype != np.uint8:
                raise ValueError("every chunk must be (N,H,W,3) uint8")
            s = slots[k % self.SLOTS]   # free: its last chunk, k - SLOTS, has been yielded
            px = a.shape[0] * a.shape[1] * a.shape[2]
            if px > s["cap"]:
                s["pin_in"] = torch.empty(px * 3, dtype=torch.uint8, pin_memory=True)
                s["dev_in"] = torch.empty(px * 3, dtype=torch.uint8, device=self.device)
                s["dev_out"] = torch.empty(px * 4, dtype=torch.uint8, device=self.device)
                s["cap"] = px
                here = torch.cuda.current_stream(self.device)   # the allocator hands memory out in this stream's order
                for st in self._streams:
                    st.wait_stream(here)
            s["shape"], s["px"] = a.shape, px
            s["pin_in"][:px * 3].numpy()[...] = a.reshape(-1)
            with torch.cuda.stream(s_in):
                s["dev_in"][:px * 3].copy_(s["pin_in"][:px * 3], non_blocking=True)
                s["up"] = s_in.record_event()

        def launch(k):
            s = slots[k % self.SLOTS]
            px, shape = s["px"], s["shape"]
            with torch.cuda.stream(s_run):
                s_run.wait_event(s["up"])
                if self.diagnose:
                    s["rec"] = self._measure(s["dev_in"][:px * 3].view(shape))
                self._launch(s["dev_in"][:px * 3].view(shape), s["dev_out"][:px * 3].view(shape),
                             s["dev_out"][px * 3:px * 4].view(shape[:3]))
                done = s_run.record_event()
            # the chunk's own page-locked block: the arrays handed out are views of it, so nothing is copied again on
            # the host; torch's host allocator takes the block back once they are dropped (and the copy has finished)
            s["pin_out"] = torch.empty(px * 4, dtype=torch.uint8, pin_memory=True)
            with torch.cuda.stream(s_out):
                s_out.wait_event(done)
                s["pin_out"].copy_(s["dev_out"][:px * 4], non_blocking=True)
                s["down"] = s_out.record_event()

        def verify(k):
            with torch.cuda.stream(s_run):
                ok = self._verify()
            if not ok:   # the chunk is still in its slot: once more, now on the fp32 tier
                launch(k)
                with torch.cuda.stream(s_run):
                    self._verify()

        def collect(k):
            s = slots[k % self.SLOTS]
            px, shape = s["px"], s["shape"]
            s["down"].synchronize()
            host = s.pop("pin_out").numpy()
            result = host[:px * 3].reshape(shape), host[px * 3:].reshape(shape[:3])
            if self.diagnose:   # the records were complete before the chunk's download began
                return result, self._frame_stats(s.pop("rec"), shape)
            return result

        # per chunk: launch it, and while the device computes do the host's share - hand out the chunk before, stage
        # and upload the chunk after - and only then wait for the device's verdict on it
        it = iter(chunks)
        try:
            nxt = next(it, None)
            if nxt is not None:
                upload(0, nxt)
            k = 0
            while nxt is not None:
                launch(k)
                if k > 0:
                    yield collect(k - 1)
                nxt = next(it, None)
                if nxt is not None:
                    upload(k + 1, nxt)
                verify(k)
                k += 1
            if k > 0:
                yield collect(k - 1)
        finally:
            for st in self._streams:   # also when the consumer stops early: nothing of this run is left in flight
                st.synchronize()


def predict_video(pipeline, read_frames, write_frame, chunk=64):
    """The loop of the reference's `predict_video` (src/unet.py:115-136) around `pipeline.run`: `read_frames` is any
    iterable of (H,W,3) uint8 BGR frames (what `cap.read()` returns), `write_frame(overlay)` is called once per frame,
    in order (the reference's `out.write(result)`); `chunk` frames go to the device at a time.  Returns (frame count,
    wall seconds).  Decoding and encoding (cv2.VideoCapture / VideoWriter) stay with the caller.  The reference's
    `putText` FPS banner on every frame (:129-130) is left out: it is text rendering over the result, and its content
    is that machine's timing."""
    chunk = int(chunk)
    if chunk <= 0:
        raise ValueError("chunk must be positive")

    def chunks():
        held = []
        for frame in read_frames:
            held.append(np.asarray(frame))
            if len(held) == chunk:
                yield np.stack(held)
                held = []
        if held:
            yield np.stack(held)

    t0 = time.perf_counter()
    count = 0
    for item in pipeline.run(chunks()):
        overlay = item[0][0] if getattr(pipeline, "diagnose", False) else item[0]
        for frame in overlay:
            write_frame(frame)
            count += 1
    return count, time.perf_counter() - t0

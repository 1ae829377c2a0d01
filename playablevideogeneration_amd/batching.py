"""Input-pipeline contract of the hot path: what the reference's `dataset/` package hands to the trainer.

    sample indices      dataset/video_dataset.py:114-149   (frame skip, newest-first stacking clamped at the start of the video)
    BatchElement/Batch  dataset/batching.py:10-95          (`to_tuple()` -> (observations, actions, rewards, dones), `.size`)
    collate             dataset/batching.py:97-112         (stack of per-observation channel-concatenated frame stacks)
    normalisation       dataset/transforms.py:90-107       (ToTensor + Normalize(0.5, 0.5): uint8 [0, 255] -> fp32 [-1, 1])
    device transforms   (opt-in) RawBatchElement / RawBatch: the distinct uint8 frames of a batch plus the (bs, T, S) list of which frame fills which
                        slot; `RawBatch.to_tuple()` runs crop, resize, normalisation and stacking as one HIP kernel (frame_pipeline.py, csrc/frames.hip)
    device decode       (opt-in) CodedBatchElement / CodedBatch: the same, with every distinct frame as the bytes of its PNG file; `CodedBatch.decode()` inflates and
                        unfilters them on the device (png_reader.py, csrc/png_read.hip) into the frames a RawBatch holds

The tensor contract lives here; the reader of the reference's on-disk format (PNG folders + pickles, dataset/video.py) and the sample
grid over videos is `playablevideogeneration_amd.video_dataset`.  `Batch.to_tuple()` moves
the tensors to the current HIP device like the reference moves them to CUDA (batching.py:67-87).
"""
from typing import List, Sequence, Tuple

import torch


def observation_indices(initial_frame: int, observations_count: int, skip_frames: int, observation_stacking: int) -> Tuple[List[int], List[List[int]]]:
    """Frame indices of one sample (video_dataset.py:131-137): observation i is frame `initial + i (skip + 1)`; its stack holds that frame
    and the `stacking - 1` preceding observations (newest first), clamped to the first frame the sampling grid can reach (`initial % (skip + 1)`)."""
    step = skip_frames + 1
    obs = [initial_frame + i * step for i in range(observations_count)]
    min_frame = initial_frame % step
    stacks = [[max(o - k * step, min_frame) for k in range(observation_stacking)] for o in obs]
    return obs, stacks


def available_samples(frames_count: int, observations_count: int, skip_frames: int) -> int:
    """video_dataset.py:92-106: samples that fit in a video of `frames_count` frames"""
    return frames_count - (observations_count + (observations_count - 1) * skip_frames) + 1


def accumulated_rewards(rewards: Sequence[float], obs_indices: Sequence[int], skip_frames: int) -> List[float]:
    """video_dataset.py:143: the reward of an observation includes the rewards of the frames skipped to reach it"""
    return [sum(rewards[max(i - skip_frames, 0):i + 1]) for i in obs_indices]


def normalize_frame(frame_uint8_hwc: torch.Tensor) -> torch.Tensor:
    """transforms.py:99-102 (ToTensor -> float -> Normalize(mean .5, std .5)): (H, W, 3) uint8 -> (3, H, W) fp32 in [-1, 1]"""
    x = frame_uint8_hwc.permute(2, 0, 1).to(torch.float32) / 255.0
    return (x - 0.5) / 0.5


class BatchElement:
    """One sampled sequence: `observations[i]` is the list of `observation_stacking` (3, H, W) tensors of observation i, newest first
    (dataset/batching.py:10-42; the frames arrive already transformed here)."""

    def __init__(self, observations, actions, rewards, dones, video=None, initial_frame_index: int = 0):
        self.observations_count = len(observations)
        self.observations_stacking = len(observations[0])
        if len(actions) != self.observations_count or len(rewards) != self.observations_count or len(dones) != self.observations_count:
            raise Exception("Missing elements in the current batch")
        self.observations, self.actions, self.rewards, self.dones = observations, actions, rewards, dones
        self.video, self.initial_frame_index = video, initial_frame_index


def is_batch_element(x) -> bool:
    return all(hasattr(x, a) for a in ("observations", "actions", "rewards", "dones")) and not torch.is_tensor(getattr(x, "observations"))


class Batch:
    """(bs, observations_count, 3 * stacking, H, W) observations + (bs, observations_count) actions / rewards / dones (batching.py:44-95)"""

    def __init__(self, observations: torch.Tensor, actions: torch.Tensor, rewards: torch.Tensor, dones: torch.Tensor, videos=None, initial_frames=None):
        self.size = actions.size(1)
        self.observations, self.actions, self.rewards, self.dones = observations, actions, rewards, dones
        self.video, self.initial_frames = videos, initial_frames

    def to_cuda(self):
        self.observations, self.actions = self.observations.cuda(non_blocking=True), self.actions.cuda(non_blocking=True)
        self.rewards, self.dones = self.rewards.cuda(non_blocking=True), self.dones.cuda(non_blocking=True)

    def to_tuple(self, cuda=True) -> Tuple:
        if cuda and torch.cuda.is_available():
            self.to_cuda()
        return self.observations, self.actions, self.rewards, self.dones

    def pin_memory(self):
        self.observations, self.actions = self.observations.pin_memory(), self.actions.pin_memory()
        self.rewards, self.dones = self.rewards.pin_memory(), self.dones.pin_memory()
        return self


def single_batch_elements_collate_fn(batch: List[BatchElement]) -> Batch:
    """batching.py:97-112: per observation the stack is concatenated along channels (newest frame first), observations are stacked along
    time, elements along the batch; actions are int32 like the reference's `dtype=torch.int`."""
    obs = torch.stack([torch.stack([torch.cat(list(stack)) for stack in el.observations], dim=0) for el in batch], dim=0)
    actions = torch.stack([torch.tensor(el.actions, dtype=torch.int) for el in batch], dim=0)
    rewards = torch.stack([torch.tensor(el.rewards) for el in batch], dim=0)
    dones = torch.stack([torch.tensor(el.dones) for el in batch], dim=0)
    return Batch(obs, actions, rewards, dones, [el.video for el in batch], [el.initial_frame_index for el in batch])


class RawBatchElement:
    """One sampled sequence before any transform (video_dataset.raw_frame_spec): `frames` are its distinct decoded frames, (h, w, 3) uint8 arrays, `stack_indices[i][s]`
    the index into them of stack position s (newest first) of observation i; annotations as in BatchElement."""

    def __init__(self, frames, stack_indices, actions, rewards, dones, spec, video=None, initial_frame_index: int = 0):
        self.observations_count = len(stack_indices)
        self.observations_stacking = len(stack_indices[0])
        if len(actions) != self.observations_count or len(rewards) != self.observations_count or len(dones) != self.observations_count:
            raise Exception("Missing elements in the current batch")
        self.frames, self.stack_indices, self.spec = frames, stack_indices, spec
        self.actions, self.rewards, self.dones = actions, rewards, dones
        self.video, self.initial_frame_index = video, initial_frame_index


class RawBatch:
    """`frames` (F, h, w, 3) uint8, `slot_src` (bs, T, S) int32 indices into them, (bs, T) actions / rewards / dones: what the host ships when the frame
    transform runs on the device.  `to_tuple()` returns what `Batch.to_tuple()` returns, bit for bit."""

    def __init__(self, frames: torch.Tensor, slot_src: torch.Tensor, actions: torch.Tensor, rewards: torch.Tensor, dones: torch.Tensor, spec, videos=None, initial_frames=None):
        self.size = actions.size(1)
        self.frames, self.slot_src, self.spec = frames, slot_src, spec
        self.actions, self.rewards, self.dones = actions, rewards, dones
        self.video, self.initial_frames = videos, initial_frames

    @property
    def n_frames(self) -> int:
        return int(self.frames.shape[0])

    @property
    def frame_hw(self) -> Tuple[int, int]:
        return int(self.frames.shape[1]), int(self.frames.shape[2])

    def staged(self) -> Tuple:
        """the tensors that carry the frames to the device"""
        return (self.frames,)

    def device_frames(self, staged: Tuple, lib=None, device=None) -> torch.Tensor:
        """(F, h, w, 3) uint8 from the copies of `staged()` on the device, on the current stream"""
        return staged[0]

    def observations(self, frames: torch.Tensor = None, slot_src: torch.Tensor = None, lib=None, device=None) -> torch.Tensor:
        """(bs, T, 3 S, H, W) fp32 on the pipeline's device, from this batch's frames (or their staged copies) on the current stream"""
        from .frame_pipeline import cached_pipeline, validate_slots
        validate_slots(self.slot_src, self.n_frames)
        frames = self.device_frames(self.staged(), lib, device) if frames is None else frames
        slot_src = self.slot_src if slot_src is None else slot_src
        h, w = self.frame_hw
        pipe = cached_pipeline(h, w, self.spec.crop, self.spec.size, self.spec.mode, self.n_frames, lib, device)
        bs, T, S = self.slot_src.shape
        return pipe(frames, slot_src).view(bs, T, 3 * S, pipe.H, pipe.W)

    def to_tuple(self, cuda=True) -> Tuple:
        obs = self.observations()
        rest = (self.actions, self.rewards, self.dones)
        if not cuda:
            return (obs.cpu(),) + rest
        if torch.cuda.is_available():
            rest = tuple(t.cuda(non_blocking=True) for t in rest)
        return (obs,) + rest

    def pin_memory(self):
        self.frames, self.slot_src = self.frames.pin_memory(), self.slot_src.pin_memory()
        self.actions, self.rewards, self.dones = self.actions.pin_memory(), self.rewards.pin_memory(), self.dones.pin_memory()
        return self


def raw_batch_elements_collate_fn(batch: List[RawBatchElement]) -> RawBatch:
    """the collate function of RawBatchElements: frames are concatenated once each, the stack indices shifted by the frames in front of their element"""
    import numpy as np
    shape = batch[0].frames[0].shape
    frames, slots = [], []
    for el in batch:
        for fr in el.frames:
            if fr.shape != shape:
                raise Exception(f"frames of different sizes in one batch: {tuple(shape)} and {tuple(fr.shape)} (such datasets keep the host transform)")
        slots.append(torch.tensor(el.stack_indices, dtype=torch.int32) + len(frames))
        frames.extend(el.frames)
    actions = torch.stack([torch.tensor(el.actions, dtype=torch.int) for el in batch], dim=0)
    rewards = torch.stack([torch.tensor(el.rewards) for el in batch], dim=0)
    dones = torch.stack([torch.tensor(el.dones) for el in batch], dim=0)
    return RawBatch(torch.from_numpy(np.stack(frames)), torch.stack(slots, dim=0), actions, rewards, dones, batch[0].spec,
                    [el.video for el in batch], [el.initial_frame_index for el in batch])


class CodedBatchElement(RawBatchElement):
    """A RawBatchElement whose `frames` are still files (video_dataset.raw_frame_spec(decode="device")): uint8 arrays of the bytes of each distinct frame's PNG -- or,
    with `codec` "jpeg", JPEG -- file, all of `frame_hw` = (h, w); `sources[k]` = (video path, frame index) of frame k, for messages."""

    def __init__(self, frames, frame_hw, sources, stack_indices, actions, rewards, dones, spec, video=None, initial_frame_index: int = 0, codec: str = "png"):
        super().__init__(frames, stack_indices, actions, rewards, dones, spec, video, initial_frame_index)
        self.frame_hw, self.sources, self.codec = tuple(frame_hw), list(sources), codec


class CodedBatch(RawBatch):
    """A RawBatch before its frames are decoded: `blob` uint8, the PNG files of the distinct frames back to back, `offsets` int32 (F + 1), `frame_hw` their common
    (h, w).  `decode()` gives the RawBatch with `frames` on the device (png_reader.PngDecoder: the compressed bytes cross the bus, the device inflates and unfilters);
    `observations()` / `to_tuple()` decode first and return what RawBatch returns, bit for bit.  A file the decoder refuses raises, naming its video and frame.
    `codec` "jpeg": the files are JPEG and jpeg_reader.JpegDecoder decodes them (Huffman decoding, IDCT, upsampling and colour on the device)."""

    def __init__(self, blob: torch.Tensor, offsets: torch.Tensor, frame_hw, sources, slot_src: torch.Tensor, actions: torch.Tensor, rewards: torch.Tensor, dones: torch.Tensor, spec,
                 videos=None, initial_frames=None, codec: str = "png"):
        super().__init__(None, slot_src, actions, rewards, dones, spec, videos, initial_frames)
        self.blob, self.offsets, self.sources, self.codec = blob, offsets, list(sources), codec
        self._hw = (int(frame_hw[0]), int(frame_hw[1]))

    @property
    def n_frames(self) -> int:
        return int(self.offsets.numel()) - 1

    @property
    def frame_hw(self) -> Tuple[int, int]:
        return self._hw

    def staged(self) -> Tuple:
        return (self.blob, self.offsets)

    def device_frames(self, staged: Tuple, lib=None, device=None) -> torch.Tensor:
        from . import metrics as M
        if self.codec == "jpeg":
            from .jpeg_reader import cached_jpeg_decoder as cached_decoder, status_error
        else:
            from .png_reader import cached_png_decoder as cached_decoder, status_error
        device = torch.device(device) if device is not None else M.device(lib)
        blob, offsets = (t.to(device, non_blocking=True) for t in staged)
        frames, status = cached_decoder(self._hw[0], self._hw[1], self.n_frames, lib, device).decode_stream(blob, offsets)
        error = status_error(status.cpu().tolist(), [f"{path} frame {index}" for path, index in self.sources])
        if error is not None:
            raise error
        return frames

    def decode(self, lib=None, device=None) -> RawBatch:
        """the RawBatch of this batch, its frames decoded on the device (on the current stream)"""
        return RawBatch(self.device_frames(self.staged(), lib, device), self.slot_src, self.actions, self.rewards, self.dones, self.spec, self.video, self.initial_frames)

    def pin_memory(self):
        self.blob, self.offsets, self.slot_src = self.blob.pin_memory(), self.offsets.pin_memory(), self.slot_src.pin_memory()
        self.actions, self.rewards, self.dones = self.actions.pin_memory(), self.rewards.pin_memory(), self.dones.pin_memory()
        return self


def coded_batch_elements_collate_fn(batch: List[CodedBatchElement]) -> CodedBatch:
    """the collate function of CodedBatchElements: the files are concatenated once each, the stack indices shifted by the frames in front of their element"""
    import numpy as np
    hw, codec = batch[0].frame_hw, batch[0].codec
    files, sources, slots = [], [], []
    for el in batch:
        if el.codec != codec:
            raise Exception(f"frames of different codecs in one batch: {codec} and {el.codec} ({el.sources[0][0]}; such datasets keep the host decoder)")
        if el.frame_hw != hw:
            raise Exception(f"frames of different sizes in one batch: {hw} and {el.frame_hw} ({el.sources[0][0]}; such datasets keep the host transform)")
        slots.append(torch.tensor(el.stack_indices, dtype=torch.int32) + len(files))
        files.extend(el.frames)
        sources.extend(el.sources)
    offsets = np.zeros(len(files) + 1, np.int64)
    np.cumsum([f.size for f in files], out=offsets[1:])
    if offsets[-1] >= 1 << 31:
        raise Exception(f"the files of one batch hold {int(offsets[-1])} bytes: more than the 32-bit offsets of the device decoder take")
    actions = torch.stack([torch.tensor(el.actions, dtype=torch.int) for el in batch], dim=0)
    rewards = torch.stack([torch.tensor(el.rewards) for el in batch], dim=0)
    dones = torch.stack([torch.tensor(el.dones) for el in batch], dim=0)
    return CodedBatch(torch.from_numpy(np.concatenate(files)), torch.from_numpy(offsets.astype(np.int32)), hw, sources, torch.stack(slots, dim=0), actions, rewards, dones,
                      batch[0].spec, [el.video for el in batch], [el.initial_frame_index for el in batch], codec)


def collate_fn_for(element):
    """the collate function of a dataset whose items look like `element`: coded or raw elements, BatchElements, or None for anything else"""
    if isinstance(element, CodedBatchElement):
        return coded_batch_elements_collate_fn
    if isinstance(element, RawBatchElement):
        return raw_batch_elements_collate_fn
    return single_batch_elements_collate_fn if is_batch_element(element) else None


def multiple_batch_elements_collate_fn(batch: List[Tuple[BatchElement]]) -> List[Batch]:
    """batching.py:114-126: one Batch per position of the tuples"""
    n = len(batch[0])
    return [single_batch_elements_collate_fn([els[i] for els in batch]) for i in range(n)]

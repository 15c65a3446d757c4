"""The frame stack the trainer consumes, restated: VecPyTorchFrameStack (pytorch-a2c-ppo-acktr/envs.py:135-165) over the
observation stream of a plain (unstacked) handle.  Every frame-stack assertion of the suite compares against this class.

Torch ops only, on whatever device it is given: on the CPU for the small batches, on the GPU for the large one (a 1536-env
float32 stack is 88 MB - not something to copy to the host every step).  No kernel of the library is involved."""
import torch


class FrameStackRef:
    def __init__(self, num_envs, nstack, frame_shape, dtype=torch.float32, device="cpu"):
        """frame_shape: one observation, channel-first (3, W, H); dtype: torch.float32 (VecPyTorch's .float(), envs.py:128)
        or torch.uint8 (the library's uint8 variant of the same stack)"""
        self.dim0 = int(frame_shape[0])   # shape_dim0, envs.py:140
        self.device, self.dtype = torch.device(device), dtype
        self.stacked = torch.zeros((num_envs, self.dim0 * nstack) + tuple(frame_shape[1:]), dtype=dtype, device=self.device)

    def _obs(self, obs):
        return torch.as_tensor(obs).to(device=self.device, dtype=self.dtype)   # uint8 -> float32 is exact

    def _flags(self, flags):
        return torch.as_tensor(flags).to(device=self.device).reshape(-1) != 0

    def reset(self, obs):
        """envs.py:158-162: everything zero, the first frame in the newest planes"""
        self.stacked.zero_()
        self.stacked[:, -self.dim0:] = self._obs(obs)
        return self.stacked

    def step(self, obs, news):
        """envs.py:149-156: shift one frame towards the front, zero the envs whose episode ended, append the new frame (for an
        env that ended: the first frame of its next episode).  A skipped env (subproc_vec_env.py:26-31: reward -99, done
        False, its current frame returned again) needs no case of its own: it is an env that is not done."""
        k = self.dim0
        self.stacked[:, :-k] = self.stacked[:, k:].clone()
        self.stacked[self._flags(news)] = 0
        self.stacked[:, -k:] = self._obs(obs)
        return self.stacked

    def partial_reset(self, obs, mask):
        """NOT part of the reference: VecPyTorchFrameStack has no partial reset.  This is the rule include/miniworld_batch.h
        documents for mwb_reset(mask) with MWB_STACK_FUSED - the call is a step for the window: the masked envs get a zeroed
        history and their first frame, the others get their re-rendered current frame appended once more."""
        return self.step(obs, mask)

"""Pinned staging buffers for the uploads of the image pipeline (ops/image_batch.py, ops/jpeg.py)."""
import torch


class Staging(object):
    """Grow-only pinned buffers handed out round-robin; a slot is reused only after the upload that read it finished."""

    def __init__(self, slots=3):
        self.slots = [[None, None] for _ in range(slots)]  # (pinned uint8 buffer, event of its last upload)
        self.turn = 0

    def take(self, nbytes):
        slot = self.slots[self.turn]
        self.turn = (self.turn + 1) % len(self.slots)
        if slot[1] is not None:
            slot[1].synchronize()
        if slot[0] is None or slot[0].numel() < nbytes:
            with torch.inference_mode(False):  # the buffer outlives the caller's inference_mode block
                slot[0] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
        return slot

    def upload(self, slot, nbytes, device):
        dev = slot[0][:nbytes].to(device, non_blocking=True)
        if slot[1] is None:
            slot[1] = torch.cuda.Event()
        slot[1].record()
        return dev

"""The fp16 activation type of the matrix-core path (shared by the plan builder, the tuner and the training ops)."""
import torch


class ActC8:
    """fp16 activation in the channel-blocked layout of the fp16 matrix-core path: physical tensor
    ``[N][ceil(C/8)][H][W][8]`` halfs (padding channels zero), ``shape`` = the logical NCHW shape."""

    def __init__(self, n: int, c: int, h: int, w: int, device) -> None:
        self.shape = torch.Size((n, c, h, w))
        self.c8_tensor = torch.zeros(n, (c + 7) // 8, h, w, 8, device=device, dtype=torch.float16)
        self.device = self.c8_tensor.device

    def data_ptr(self) -> int:
        return self.c8_tensor.data_ptr()

    def to_nchw(self) -> torch.Tensor:
        """fp32 NCHW copy (tests / debugging)."""
        n, c, h, w = self.shape
        return self.c8_tensor.permute(0, 1, 4, 2, 3).reshape(n, -1, h, w)[:, :c].float().contiguous()

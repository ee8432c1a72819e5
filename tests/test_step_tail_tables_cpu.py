"""The host tables of the device-resident step tail (utils/step_tail.py): entry i is the fp32 value the host-driven step passes to
the update kernel at ``global_step == i``."""
import numpy as np
import pytest

from mindpose_amd.utils.lr import WarmupCosineDecayLR, WarmupMultiStepDecayLR
from mindpose_amd.utils.step_tail import ARGS_DTYPE, STATE_DTYPE, adam_aux_table, lr_table


@pytest.mark.parametrize("schedule", [WarmupMultiStepDecayLR(1e-3, 4, 5, [3, 4], warmup=3), WarmupCosineDecayLR(5e-4, 3, 4, warmup=2)],
                         ids=["multi_step", "cosine"])
def test_lr_table_is_the_schedule_in_fp32(schedule):
    table = lr_table(schedule, schedule.total_steps)
    assert table.dtype == np.float32 and table.shape == (schedule.total_steps,)
    for i in range(schedule.total_steps):
        assert table[i] == np.float32(schedule(i)), i
    assert len(set(table.tolist())) > 2  # warm-up and decay are both in the table


def test_constant_lr_gives_one_entry():
    table = lr_table(1e-3, 100)
    assert table.dtype == np.float32 and table.shape == (1,) and table[0] == np.float32(1e-3)


def test_adam_aux_table():
    b1, b2 = 0.9, 0.999
    table = adam_aux_table(b1, b2, 37)
    assert table.dtype == np.float32 and table.shape == (37, 2)
    for i in range(37):
        assert table[i, 0] == np.float32(b1 ** (i + 1)) and table[i, 1] == np.float32(b2 ** (i + 1)), i


def test_bad_lengths():
    with pytest.raises(ValueError):
        lr_table(lambda i: 1.0, 0)
    with pytest.raises(ValueError):
        adam_aux_table(0.9, 0.999, 0)


def test_block_layouts_match_the_header():
    # mp_train_tail_state: double + 4 x int64; mp_step_args: int32 + 5 x float (include/mindpose_hip.h)
    assert STATE_DTYPE.itemsize == 40 and [STATE_DTYPE.fields[n][1] for n in STATE_DTYPE.names] == [0, 8, 16, 24, 32]
    assert ARGS_DTYPE.itemsize == 24 and [ARGS_DTYPE.fields[n][1] for n in ARGS_DTYPE.names] == [0, 4, 8, 12, 16, 20]

"""Pin tests/golden/tiny_f4_8_validate.npz (the reference's own validate(), tests/golden/make_golden_val.py) to the CPU
oracle, so that oracle and fixture cannot drift apart.  CPU only."""
import os

import numpy as np
import torch

from oracle import unet_oracle as O
from unet_lane_detection_amd import state as S


def test_validate_fixture_matches_oracle(golden_dir):
    g = np.load(os.path.join(golden_dir, "tiny_f4_8_validate.npz"), allow_pickle=False)
    assert g["input"].shape == (6, 3, 32, 32) and g["mask_u8"].shape == (6, 1, 32, 32) and g["mask_u8"].dtype == np.uint8
    assert set(np.unique(g["mask_u8"])) <= {0, 255}
    # the condition the generator asserts: no pixel within 1e-4 of the threshold
    assert np.abs(g["logits"]).min() >= 1e-4 and abs(float(g["min_abs_logit"]) - np.abs(g["logits"]).min()) < 1e-12
    sd = O.to_torch_state(S.seeded_state_dict([4, 8], seed=1))
    x = torch.from_numpy(g["input"])
    t = torch.from_numpy(g["mask_u8"].astype(np.float32) / 255.0)
    with torch.no_grad():
        logits = O.forward(sd, x, training=False)
    np.testing.assert_allclose(logits.numpy(), g["logits"], rtol=0, atol=2e-5)   # fp32 reassociation noise
    losses, dices = [], []
    for i in range(3):
        lg, tb = logits[2 * i:2 * i + 2], t[2 * i:2 * i + 2]
        total, bce, dice = O.bce_dice_loss(lg, tb, 0.5, 0.5, pos_weight=3.0)
        assert abs(total.item() - g["batch_total"][i]) < 2e-5
        assert abs(bce.item() - g["batch_bce"][i]) < 2e-5 and abs(dice.item() - g["batch_dice_loss"][i]) < 2e-5
        d = O.compute_dice(torch.sigmoid(lg) > 0.5, tb).item()
        assert abs(d - g["batch_dice"][i]) < 1e-6
        losses.append(total.item())
        dices.append(d)
    # the reference averages per-batch values over the batches (README.md:2106-2110)
    assert abs(np.mean(losses) - float(g["avg_loss"])) < 2e-5
    assert abs(np.mean(dices) - float(g["avg_dice"])) < 1e-6
    assert abs(g["batch_total"].mean() - float(g["avg_loss"])) < 1e-12
    assert abs(g["batch_dice"].mean() - float(g["avg_dice"])) < 1e-12

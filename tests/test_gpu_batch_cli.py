"""main_train -b 2 end to end on the GPU: the fit honours the batch size in its schedule, its log and its checkpoint."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_train_cli_with_batch_2(tmp_path, monkeypatch):
    """12 synthetic frames at 40 x 60, 4 epochs, -b 2: six optimiser steps per epoch in the log, PSNR rising, Adam's step 24 in the
    checkpoint (not 48), no step skipped."""
    from orn_amd import main_train
    flags = ('-e 4 --lower_width 96 --num_blocks 1 --dataset bunny --frame_gap 1 --embed 1.25_40 --stem_dim_num 32_1 '
             '--reduction 2 --fc_hw_dim 2_3_26 --expansion 1 --single_res --loss_type Fusion6 --warmup 0.2 --lr_type cosine '
             '--strides 5 2 2 --conv_type conv -b 2 --lr 0.0005 --norm none --act swish --outf b2_t --branch_type ERB '
             '--synthetic 12 --eval_freq 2').split()
    monkeypatch.chdir(tmp_path)
    best = main_train.train(main_train.parse_args(flags))
    assert list(best) == ['synthetic0']
    outf = tmp_path / 'result' / 'b2_t'
    log = (outf / 'rank0.txt').read_text()
    epochs = re.findall(r'Epoch\[\d+/4\], lr:\S+ PSNR: ([0-9.]+), .*steps: (\d+),', log)
    print(epochs)
    assert len(epochs) == 4 and all(int(s) == 6 for _, s in epochs)
    psnr = [float(p) for p, _ in epochs]
    assert psnr[-1] > psnr[0]
    ck = torch.load(outf / 'model_latest.pth', map_location='cpu', weights_only=True)
    assert ck['epoch'] == 4 and float(ck['optimizer']['state'][0]['step']) == 24
    assert 'steps skipped' not in log

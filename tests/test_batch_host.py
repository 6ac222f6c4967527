"""Host side of -b / --batchSize (no GPU): the schedule of an epoch with B frames per optimiser step (main_train.py:205-254 with
DataLoader(batch_size=B, drop_last=True)), and the places that must refuse a batch they cannot honour."""
import inspect

import pytest
import torch

FLAGS = ('-e 10 --warmup 0.2 --lr 0.0005 --lr_type cosine --fc_hw_dim 2_3_26 --strides 5 2 2 --lower_width 96 '
         '--branch_type ERB --synthetic 13').split()


def _args(extra=()):
    from orn_amd import main_train
    return main_train.parse_args(FLAGS + list(extra))


def _order(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed)).tolist()


def test_epoch_entries_drop_the_last_partial_batch():
    from orn_amd import main_train
    args = _args(['-b', '4'])
    order = _order(13, 3)
    entries = main_train.epoch_entries(order, 2, 13, 4, args)
    assert len(entries) == 12                                     # 13 // 4 = 3 steps of 4 frames
    assert [e[0] for e in entries] == order[:12] and order[12] not in [e[0] for e in entries]
    for i in range(3):
        batch = entries[4 * i:4 * i + 4]
        assert len({(s, lr) for _, s, lr in batch}) == 1          # one Adam step and one lr per batch
        assert batch[0][1] == 2 * 3 + i + 1                       # Adam advances by one per BATCH: 3 steps per epoch
    # steps skipped by an engine that a precision fall-back replaced come off the step numbers
    carried = main_train.epoch_entries(order, 2, 13, 4, args, skipped_carry=2)
    assert [e[1] for e in carried] == [e[1] - 2 for e in entries]


@pytest.mark.parametrize('epoch', [1, 5], ids=['in_warmup', 'past_warmup'])
def test_batch_lr_is_the_reference_schedule_at_the_batch_index(epoch):
    """adjust_lr(epoch, i, len(dataset)): `i` is the batch index, data_size stays the FRAME count (main_train.py:247)."""
    from oracle import cpu_ref
    from orn_amd import main_train
    args = _args(['-b', '4'])
    assert args.warmup == 2
    entries = main_train.epoch_entries(_order(13, 4), epoch, 13, 4, args)
    for i in range(3):
        want = cpu_ref.adjust_lr_value(epoch, i, 13, args.lr, args.epochs, args.warmup, args.lr_type)
        assert entries[4 * i][2] == want and entries[4 * i + 3][2] == want
    assert (epoch < args.warmup) == (entries[0][2] < entries[-1][2])          # ramping up inside the warm-up, decaying after


def test_batch_one_reproduces_the_single_frame_schedule():
    from orn_amd import main_train, utils
    args = _args()
    assert args.batchSize == 1
    for epoch, n, carry in [(0, 13, 0), (3, 13, 1), (7, 5, 0)]:
        order = _order(n, epoch)
        want = [(f, epoch * n + i + 1 - carry, utils.lr_value(epoch % args.epochs, i, n, args)) for i, f in enumerate(order)]
        assert main_train.epoch_entries(order, epoch, n, 1, args, carry) == want


def test_a_batch_larger_than_the_video_is_an_error():
    from orn_amd import main_train
    main_train.check_batch_size(13, 13)
    with pytest.raises(ValueError, match='larger than the 13 training frames'):
        main_train.check_batch_size(14, 13)
    with pytest.raises(ValueError, match='batchSize'):
        main_train.check_batch_size(0, 13)


def test_finetune_refuses_a_batch():
    """main_eval --finetune steps one frame at a time: -b 2 is refused (before anything is loaded), not ignored."""
    from orn_amd import main_eval
    with pytest.raises(ValueError, match='--finetune with -b'):
        main_eval.main(FLAGS + ['--finetune', '-b', '2', '--outf', 'no_such_run'])


def test_run_takes_a_batch():
    from orn_amd import engine
    sig = inspect.signature(engine.TrainEngine.run)
    assert list(sig.parameters)[1:] == ['n_steps', 'graph', 'batch'] and sig.parameters['batch'].default == 1

"""main_eval's command line: `--decoder` selects the decode path of the evaluation (eager module forward, or the native engine)."""
import pytest


def test_decoder_flag_defaults_to_eager():
    from orn_amd import main_eval
    p = main_eval.eval_parser()
    assert p.parse_args([]).decoder == 'eager'
    assert p.parse_args(['--decoder', 'eager']).decoder == 'eager'
    args = p.parse_args(['--decoder', 'engine', '--precision', 'bf16', '--dump_images'])
    assert args.decoder == 'engine' and args.precision == 'bf16' and args.dump_images
    with pytest.raises(SystemExit):
        p.parse_args(['--decoder', 'triton'])

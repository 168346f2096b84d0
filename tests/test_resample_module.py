"""What ``transforms.Resample`` / ``ResampleStream`` and the ``sample_rate`` arguments decide on the host, without a GPU and without the built
library: the constructor's geometry and refusals, the no-CPU-path rule, and that the new arguments default to today's calls."""
import inspect

import pytest
import torch

import resample_cases as rc


@pytest.fixture(scope="module")
def transforms():
    from audio_denoising_amd import transforms          # (constructing a transform loads no library and needs no device)
    return transforms


@pytest.mark.parametrize("orig,new", rc.PAIRS + ((11025, 16000),))
def test_constructor_geometry_is_the_restatements(transforms, orig, new):
    r, geo = transforms.Resample(orig, new), rc.Geometry(orig, new)
    assert (r.o, r.n, r.width, r.taps, r.delay_blocks) == (geo.o, geo.n, geo.width, geo.KW, geo.D)
    assert [r.out_len(L) for L in (1, geo.o, 1009)] == [geo.out_len(L) for L in (1, geo.o, 1009)]
    s = transforms.ResampleStream(r, 4)
    assert (s.delay, s.history) == (geo.D * geo.n, geo.H)


def test_constructor_refusals(transforms):
    R = transforms.Resample
    for bad in (dict(resampling_method="linear"), dict(orig_freq=16000.5), dict(lowpass_filter_width=0), dict(rolloff=0.0), dict(rolloff=1.5), dict(orig_freq=0),
                dict(new_freq=-3)):
        with pytest.raises(ValueError):
            R(**{**dict(orig_freq=48000, new_freq=16000), **bad})
    with pytest.raises(TypeError):
        R(48000, 16000, dtype=torch.int32)
    for o, n in ((1025, 1), (3, 1031)):
        with pytest.raises(NotImplementedError):
            R(o, n)
    with pytest.raises(NotImplementedError):
        R(1024, 1023, lowpass_filter_width=400)
    with pytest.raises(ValueError):
        transforms.ResampleStream(R(16000, 16000), 2)
    with pytest.raises(ValueError):
        transforms.ResampleStream(R(48000, 16000), 0)
    assert inspect.signature(R.__init__).parameters["dtype"].kind is inspect.Parameter.KEYWORD_ONLY


def test_there_is_no_cpu_path(transforms):
    r = transforms.Resample(48000, 16000)
    with pytest.raises(RuntimeError, match="CUDA"):
        r(torch.zeros(2, 30))
    with pytest.raises(RuntimeError, match="CUDA"):
        transforms.ResampleStream(r, 2).push(torch.zeros(2, 30))
    with pytest.raises(RuntimeError):
        transforms.ResampleStream(r, 2).flush()


def test_rate_arguments_default_to_todays_calls(transforms):
    from audio_denoising_amd.pipeline import Denoiser
    assert inspect.signature(Denoiser.denoise_clip).parameters["sample_rate"].default is None
    assert inspect.signature(Denoiser.denoise_clips).parameters["sample_rates"].default is None

"""Time-domain baseline defenses of the attack drivers, at the reference's module path (transforms/time_defense.py:8-157):
TimeDomainDefense with AS (average smoothing) and MS (median smoothing).  Signatures, defaults, accepted shapes, _get_name() strings and
the NotImplementedError for an unknown type are the reference's; so is MS's zero padding (its comment says "replicate", its code pads
with 0).  AT (audio turbulence) is reachable from no driver and is not provided.

backend = 'hip' runs the engine's kernels (dmad_wave_smooth, differentiable through dmad_wave_smooth_vjp), 'host' the reference's torch
ops on whatever device the input lives on.  Default: 'hip' for CUDA input when an engine is at hand, 'host' otherwise."""
from . import _wave_design as wd


class TimeDomainDefense():

    def __init__(self, defense_type: str, *args, backend=None, engine=None) -> None:
        self.defense_type = defense_type
        self.backend, self.engine = backend, engine

    def __call__(self, x, *args):
        if self.defense_type == 'AT':
            output = AT(x)
        elif self.defense_type == 'AS':
            output = AS(x, backend=self.backend, engine=self.engine)
        elif self.defense_type == 'MS':
            output = MS(x, backend=self.backend, engine=self.engine)
        else:
            raise NotImplementedError(f'Unknown defense type: {self.defense_type}!')
        return output

    def _get_name(self, *args):
        if self.defense_type == 'AT':
            name = 'Audio_Turbulence'
        elif self.defense_type == 'AS':
            name = 'Average_Smoothing'
        elif self.defense_type == 'MS':
            name = 'Median_Smoothing'
        else:
            raise NotImplementedError(f'Unknown defense type: {self.defense_type}!')
        return name

    def engine_defense(self, x=None):
        """The defense as Engine.defense_query_logits takes it (AcousticSystem.query's one-call path)."""
        if self.defense_type not in ('AS', 'MS'):
            raise NotImplementedError(f'Unknown defense type: {self.defense_type}!')
        return dict(kind=self.defense_type, window=3)


def AT(audio, param=25, same_size=True):
    raise NotImplementedError('AT (Audio_Turbulence) is not provided: no attack driver reaches it')


def _smooth(audio, kind, window, backend, engine):
    rows, ori_shape = wd.as_rows(audio)
    which, eng = wd.pick_backend(rows, backend, engine)
    if which == 'hip':
        from dmad_hip.autograd import WaveSmoothHIP
        out = WaveSmoothHIP.apply(rows.contiguous().float(), eng, kind, window).to(rows.dtype)
    else:
        out = wd.host_mean(rows, window) if kind == 0 else wd.host_median(rows, window)
    return out.reshape(ori_shape)


def AS(audio, param=3, same_size=True, *, backend=None, engine=None):
    kernel_size = param
    assert kernel_size % 2 == 1
    return _smooth(audio, 0, kernel_size, backend, engine)


def MS(audio, param=3, same_size=True, *, backend=None, engine=None):
    r"""
    Apply median smoothing to the 1D tensor over the given window.
    """
    return _smooth(audio, 1, param, backend, engine)

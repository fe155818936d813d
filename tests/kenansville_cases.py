"""What the Kenansville and wave-FFT tests share: the fixture's model and how its weights are rebuilt from the seed the fixture records
(tests/golden/make_golden_kenansville.py: model_weight), and the fixture that stops a GPU session after a HIP error."""
import pytest
import torch


class StridedAverageLinear(torch.nn.Module):
    """The fixture's model: feature f is the mean of the samples f, f + F, f + 2F, ...; logits = features @ W^T."""

    def __init__(self, weight):
        super().__init__()
        self.weight = torch.nn.Parameter(weight, requires_grad=False)

    def forward(self, x):
        F = self.weight.shape[1]
        return x[:, 0].reshape(x.shape[0], -1, F).mean(1) @ self.weight.t()


def fixture_weight(g):
    """The [classes, features] weights of kenansville.npz from its seed and gain, checked against the corner and the sum it records."""
    classes, features = (int(v) for v in g['model_shape'])
    W = torch.randn(classes, features, generator=torch.Generator().manual_seed(int(g['model_seed']))) * float(g['model_gain'])
    assert torch.equal(W[:, :8], torch.from_numpy(g['weight_corner'])) and float(W.double().sum()) == float(g['weight_sum']), \
        'torch.randn no longer gives the weights the fixture was recorded with'
    return W


@pytest.fixture(autouse=True)
def stop_after_a_gpu_fault():
    """A failed assertion is one test's business; a HIP error after a test is the device's: nothing more is started on it."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:      # noqa: BLE001
        pytest.exit('HIP error after a test, stopping the session: %s' % e, returncode=3)

"""Host half of the caller-stream tests: the decoy and the real input of every late-input case of tests/stream_cases.py have answers at
least 1e3 bars apart (a stale read on the device cannot pass tests/test_gpu_caller_stream.py), and a stream handle of 0 -- the
null / legacy stream -- is refused by Context before the library is asked for anything."""
import numpy as np
import pytest

from tests import stream_cases as sc


@pytest.mark.parametrize("name", ["expv_device_b", "arnoldi_device_b", "csr_values", "update_values", "dense_operator", "exponential", "phi",
                                  "mul", "gemv_block"])
def test_decoy_and_real_input_are_far_apart(name):
    case = sc.late_cases()[name]
    assert set(sc.late_cases()) == {"expv_device_b", "arnoldi_device_b", "csr_values", "update_values", "dense_operator", "exponential",
                                    "phi", "mul", "gemv_block"}
    x0, x1 = case.x
    assert np.any(np.asarray(x0) != 0) and np.asarray(x0).shape == np.asarray(x1).shape and np.isfinite(np.asarray(x0)).all()
    sep = case.separation()
    print("%-18s separation %.3e, bar %.1e (%s)" % (name, sep, case.bar, case.mode))
    assert sep > 0 and sep >= 1e3 * case.bar, (name, sep, case.bar)


class _NullStream:
    cuda_stream = 0


@pytest.mark.parametrize("stream", [_NullStream(), 0], ids=["object_with_cuda_stream_0", "integer_0"])
def test_the_null_stream_is_refused(stream, monkeypatch):
    import expv_mi_loader
    eu = expv_mi_loader.load()
    created = []
    monkeypatch.setattr(eu.api.L, "load", lambda: created.append(1) or pytest.fail("the library was reached"))
    with pytest.raises(ValueError) as e:
        eu.Context(stream=stream)
    msg = str(e.value)
    assert "null" in msg and "legacy" in msg and "cannot be adopted" in msg and "None" in msg and "private" in msg, msg
    assert not created

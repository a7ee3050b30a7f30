"""A backbone learns something: FNO2DModule, trained for 100 steps through the HIP training path on device-generated
Navier-Stokes trajectories (synthetic.NavierStokes2D), predicts held-out next frames better than persistence and better than it
did before training.

With oracle/restate/fno.py on the CPU, the same data law and these settings the held-out one-step MSE reached 0.53-0.64 of the
persistence MSE between steps 25 and 150 (persistence rel-L2 0.096; the model at initialisation 1.39 x persistence); the run
began to overfit after step 150 and a pool of 32 trajectories does not beat persistence at all -- hence 256 trajectories and
100 steps.  The HIP path on MI355X: 0.635 of persistence after 100 steps, 1.556 before."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_fno_beats_persistence_on_held_out_trajectories():
    from dlwp_benchmark_amd import losses
    from dlwp_benchmark_amd import optim as O
    from dlwp_benchmark_amd.models import FNO2DModule
    from dlwp_benchmark_amd.synthetic import NavierStokes2D

    gen = NavierStokes2D(n=32, substeps=250, device=DEV)
    raw = gen.trajectories(288, 9)[2]
    assert raw.shape == (288, 9, 1, 32, 32) and bool(torch.isfinite(raw).all())
    prog = raw / raw[:256].std()
    x_train, y_train = gen.windows(prog[:256], 2, 1)            # [2048, 2, 1, 32, 32], [2048, 1, 1, 32, 32]
    x_held, y_held = gen.windows(prog[256:], 2, 1)
    assert x_train.shape == (2048, 2, 1, 32, 32) and y_held.shape == (256, 1, 1, 32, 32)

    torch.manual_seed(0)                                        # torch's default convolution init
    model = FNO2DModule(n_modes=[12, 12], constant_channels=0, prescribed_channels=0, prognostic_channels=1, hidden_channels=32,
                        lifting_channels=64, projection_channels=64, n_layers=4, context_size=1)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.is_complex():                                  # the spectral weights: normal, std 0.088 per part
                p.copy_(torch.view_as_complex(torch.randn(*p.shape, 2, generator=g) * 0.088))
    model = model.to(DEV)

    def held_out_mse():
        """through the training path's forward, as the steps below: the inference path (the persistent rollout kernel) takes
        widths that are multiples of 64 only, and the network has no layer that behaves differently under .train()"""
        err = 0.0
        for s in range(0, x_held.shape[0], 64):
            out = model(prognostic=x_held[s:s + 64]).detach()
            err += float(torch.sum((out - y_held[s:s + 64]) ** 2))
        return err / y_held.numel()

    persistence = float(torch.mean((x_held[:, :1] - y_held) ** 2))
    model.train()
    before = held_out_mse()
    criterion = losses.CustomMSELoss()
    optimizer = O.FusedAdamW(list(model.parameters()), lr=1e-3, weight_decay=0.0)
    order = torch.randperm(x_train.shape[0], generator=g)
    for step in range(100):
        idx = order[(step * 32) % 2048:(step * 32) % 2048 + 32].to(DEV)
        optimizer.zero_grad()
        y = model(prognostic=x_train[idx])
        assert y.requires_grad
        loss = criterion(y, y_train[idx])
        loss.backward()
        optimizer.step()
    after = held_out_mse()
    print(f"FNO on Navier-Stokes 32x32: held-out one-step MSE {after:.4e} after 100 steps, {before:.4e} before, persistence "
          f"{persistence:.4e}: {after / persistence:.3f} of persistence ({before / persistence:.3f} before)")
    assert after < persistence
    assert after < before

"""flow-timesnet_amd — MI355X-native (gfx950) TimesBlock forward path for
Flow-TimesNet, behind the reference's own PyTorch-module API.

Sub-modules
-----------
``synth``            seeded synthetic weights / inputs (numpy only)
``lib``              ctypes binding of ``csrc/libflowtimes_hip.so`` (the C-ABI in ``include/flowtimes.h``)
``pack``             host-side weight folding/packing for the HIP kernels
``models.timesnet``  drop-in mirrors of the reference modules
``models.shell``     mirror of the TimesNet model shell; HIP embedding / head kernels around the blocks
``dist``             batch-sharded multi-GPU forward (RCCL via torch.distributed)
``forecast``         recursive forecasting with the window state on the device (eager or one HIP graph);
                     ``forecast_sample_paths``: the same recursion fed with draws, P paths as one batch
``score``            NB likelihood and sMAPE of a forecast on the device: ``negative_binomial_nll``, ``ForecastScorer``;
                     the distribution itself: ``nb_cdf``, ``nb_quantiles``, ``prediction_interval``, ``interval_metrics``;
                     sample paths: ``nb_sample`` (counter-based Philox, CDF inversion), ``sample_uniforms``,
                     ``path_quantiles``; summaries of the paths in one kernel pass: ``path_summary`` (order statistics,
                     mean and sample CRPS of window sums or maxima), ``path_metrics``
``nbdist``           the distribution's reference in torch ops, on any device: the NB CDF, the one bracketed quantile
                     search behind ``nb_quantiles`` and ``nb_sample``, Philox4x32-10 and ``sample_uniforms``; pure
                     functions without a backend choice (``score`` re-exports what callers use)
``windows``          ``DeviceWindows``: the batches of a rolling-origin backtest formed on the device from the wide
                     table, in the order and shapes of the reference's ``SlidingWindowDataset`` + ``DataLoader``; with
                     ``shuffle`` / ``drop_last`` / ``seed`` / ``augment`` the training loader: shuffled epochs, time
                     shift and noise as pure functions of ``(seed, epoch)``
``table``            the table's preparation on the device: ``series_features`` (the reference's static features, the
                     full-history spectrum on the matrix pipe), ``SeriesScaler`` (fit, transform, inverse and clip),
                     ``holdout_rows`` / ``rolling_rows``
``fit``              adapting a checkpoint to new data: ``nb_nll_grad``, the loss and its closed-form gradients with
                     respect to rate and dispersion (fp64 inside, one kernel pass), and ``negative_binomial_nll`` as
                     an autograd node over them; ``head_nll``, the heads with their backward on the device, and
                     ``refit_heads``, the loop over ``TimesNet.head_inputs``
``graph``            HIP-graph capture / replay of an inference forward
"""
from . import synth  # noqa: F401


def __getattr__(name):  # lazy: keeps `import flow_timesnet_amd.synth` torch-free
    import importlib

    if name in ("lib", "pack", "models", "dist", "grouping", "runtime", "graph", "forecast", "score", "nbdist", "windows",
                "table", "fit"):
        return importlib.import_module(f"{__name__}.{name}")
    raise AttributeError(name)

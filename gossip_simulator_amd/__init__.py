"""gossip_simulator_amd -- MI355X-native engine for the broadcast round loop of
go-distributed/gossip_simulator (simulator.go).

Layers:
  include/gossip.h          C ABI (the drop-in seam; cgo binding in INTEGRATION.md)
  csrc/gs_broadcast.hip     tick kernels: delivery, infection, crash, stats
  csrc/gs_win_*.hip         window engine (default), one file per stage: units, expand,
                            part (partition), resolve, shard; shared helpers in gs_win_dev.h
  csrc/gs_wave.h            wave and block primitives shared by the kernels
  csrc/gs_pp_*.hip          push-pull rounds (extension, config C5), one file per round mode or
                            preparation step: dense, early, round, defer, rev (reverse table), fmask;
                            what they share in gs_pp_dev.h
  csrc/gs_pushpull_trials.hip  batched push-pull trials: a workgroup per trial, state in LDS
  csrc/gs_rumor.hip         rumor mongering rounds (extension): a list engine over the hot set;
                            the pull variants: a dense engine over bitsets
  csrc/gs_rumor_trials.hip  batched rumor trials: a workgroup per trial, state in LDS, every mode
                            dense over bitsets (plan: gs_rmt_plan.h)
  csrc/gs_rumorset.hip      concurrent push-pull rumors (gs_create_rumorset): up to 64 broadcasts over
                            one table in one pass, a bit per rumor in a u64 per node; a dense engine
  csrc/gs_rumorset_cap.hip  bounded rumor sets: the round under a payload cap per message, late starts
                            (selection: gs_pick.h, plain C++ for host and device)
  csrc/gs_overlay.hip       overlay construction (makeup/breakup) on the GPU
  csrc/gs_api.cpp           C ABI entry points: argument checks, dispatch by context kind
  csrc/gs_ctx.h, gs_ctx.cpp the context behind the ABI: set-up and release of every kind
  csrc/gs_peers.cpp         peer tables, the overlay into them, failure masks
  csrc/gs_windows.cpp       host side of the unsharded flood: host- and device-driven windows
  csrc/gs_shards.cpp        host side of flood node-range shards and their exchanges
  csrc/gs_pushpull_host.cpp host side of push-pull: sparse rounds, shards, batched trials
  csrc/gs_rumor_host.cpp    host side of rumor mongering: buffers, its launchers for the round loop
  csrc/gs_median_host.cpp   host side of median-counter push-pull: the same, and its batched trials
  csrc/gs_rumorset_host.cpp host side of a rumor set: refusals, buffers, its launchers and row hook for
                            the round loop, per-rumor results
  csrc/gs_round_host.cpp    the round loop those three share: step, read-back, accounting, gs_run's stop rule
  csrc/gs_trials_host.cpp   the step and run loops the batched-trial engines share
  csrc/gs_devmem.cpp        process-wide cache of large device blocks (gs_trim)
  csrc/gossip_sim.cpp       CLI with the reference's flags and stdout
  engine.py                 Python host API (ctypes)
  peers.py                  injected peer-table file format
  dist.py                   multi-GPU sharding (trials; node ranges)
"""
from ._lib import (GS_RUN_COVERED, GS_RUN_MAX_TICKS, GS_RUN_QUIESCENT,  # noqa: F401
                   GossipError, load)
from .engine import (Config, Simulator, covered, median_trials_max_n, memory_stats,  # noqa: F401
                     pp_trials_max_n, pp_trials_max_n_masked, rumor_trials_max_n, trim)

__all__ = ["Config", "Simulator", "GossipError", "covered", "load", "trim", "memory_stats", "pp_trials_max_n",
           "pp_trials_max_n_masked", "rumor_trials_max_n", "median_trials_max_n", "GS_RUN_COVERED",
           "GS_RUN_QUIESCENT", "GS_RUN_MAX_TICKS"]

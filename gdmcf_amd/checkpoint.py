"""Checkpoint / resume for the diffusion trainer.

The reference only pickles the module on the best validation epoch (`torch.save(model, .../model.pth)`,
main.py:373-375) and cannot resume: the AdamW moments and the importance-sampling history
(`Lt_history`, `Lt_count`) are lost.  `save_checkpoint` stores everything a bit-exact resume needs:

* "model": the `state_dict` (reference key names, so it also loads into the reference's DNN);
* "optimizer": its `state_dict` (moments and step counts);
* "engine": `engine.seed` / `engine.offset`, the Philox key and position of the denoiser engine's draws (dropout, the x0
  target's in-kernel noise, the one-hot class draws);
* "diffusion": `Lt_history`, `Lt_count`, and the position of every stream the diffusion object draws from itself --
  `_ts_calls` (timesteps), `_q_calls` (`q_sample`), `_randn_calls` (the eps target's normals and the reverse loop's sampling
  noise), `_noise_calls` (`apply_noise` and the degree-guided graph picks) -- with the seed those draws are keyed on
  (`GaussianDiffusion.draw_seed()`).  A resumed run keeps that seed, whatever `torch.manual_seed` its process ran;
* "epoch" and "extra", the caller's.

What the caller still owns (hand it through `extra` or save it next to the checkpoint): the data loader's generator
(`extra={"loader": g.get_state()}`), `lightgcn.BPRTrainer.state_dict()`, and torch's global generators when `rng == "torch"`.
A `graph.GraphedTrainStep` is closed before saving: `close()` hands its device counters back to the objects saved here.
Checkpoints written before the diffusion's counters were complete load as they did: a missing counter is 0, a missing seed
means torch's."""
import torch


# key in the saved state -> the diffusion's attribute: every `_*_calls` counter gaussian_diffusion.py keeps
_COUNTERS = {"ts_calls": "_ts_calls", "q_calls": "_q_calls", "randn_calls": "_randn_calls", "noise_calls": "_noise_calls"}


def diffusion_state(diffusion):
    state = {"Lt_history": diffusion.Lt_history.detach().cpu().clone(),
             "Lt_count": diffusion.Lt_count.detach().cpu().clone(),
             "seed": int(diffusion.draw_seed())}
    state.update({key: int(getattr(diffusion, attr, 0)) for key, attr in _COUNTERS.items()})
    return state


def load_diffusion_state(diffusion, state):
    diffusion.Lt_history.copy_(state["Lt_history"].to(diffusion.Lt_history.device))
    diffusion.Lt_count.copy_(state["Lt_count"].to(diffusion.Lt_count.device))
    for key, attr in _COUNTERS.items():
        setattr(diffusion, attr, int(state.get(key, 0)))
    seed = state.get("seed")
    diffusion._draw_seed = None if seed is None else int(seed)


def save_checkpoint(path, model, diffusion=None, optimizer=None, epoch=0, extra=None):
    eng = model._engine
    ckpt = {"model": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "epoch": int(epoch),
            "engine": {"seed": eng.seed, "offset": eng.offset} if eng is not None else None,
            "diffusion": diffusion_state(diffusion) if diffusion is not None else None,
            "optimizer": optimizer.state_dict() if optimizer is not None else None, "extra": extra}
    torch.save(ckpt, path)


def load_checkpoint(path, model, diffusion=None, optimizer=None, map_location=None):
    ckpt = torch.load(path, map_location=map_location, weights_only=False)
    model.load_state_dict(ckpt["model"])
    if ckpt.get("engine") is not None:
        model.engine.seed, model.engine.offset = ckpt["engine"]["seed"], ckpt["engine"]["offset"]
    if diffusion is not None and ckpt.get("diffusion") is not None:
        load_diffusion_state(diffusion, ckpt["diffusion"])
    if optimizer is not None and ckpt.get("optimizer") is not None:
        optimizer.load_state_dict(ckpt["optimizer"])
    return ckpt["epoch"], ckpt.get("extra")

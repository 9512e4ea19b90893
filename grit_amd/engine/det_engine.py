"""One optimisation step of detector pre-training (reference engine/det_solver.py:58-110, without its hook machinery)."""
import torch


def weighted_loss(loss_dict, weight_dict):
    """The sum the detector is trained on: every entry of loss_dict that weight_dict names, times its weight."""
    return sum(loss_dict[k] * weight_dict[k] for k in loss_dict if k in weight_dict)


def train_step(model, criterion, optimizer, samples, targets, max_norm=0.1):
    """forward -> criterion -> weighted sum over criterion.weight_dict -> backward -> gradient clipping (max_norm > 0) -> step.
    Returns (total, loss_dict): device tensors, nothing is read back here."""
    model.train()
    criterion.train()
    loss_dict = criterion(model(samples), targets)
    total = weighted_loss(loss_dict, criterion.weight_dict)
    optimizer.zero_grad(set_to_none=True)
    total.backward()
    if max_norm and max_norm > 0:
        torch.nn.utils.clip_grad_norm_([p for p in model.parameters() if p.requires_grad], max_norm)
    optimizer.step()
    return total.detach(), {k: v.detach() for k, v in loss_dict.items()}

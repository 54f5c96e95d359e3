"""Pretrain-stack MoE layers (drop-in for moe_pretrain_model/layers/moe + layers/cvmm.py)."""
from .register import register_moe, get_moe, MOE_REGISTRY
from .framework_layers import LoggingLayer, RegularizedLayer, OncePerIterLayer
from .cvmm import CVMMSel, cvmm, cvmm_prepare_sel2
from .moe import MoE
from .smoe import SMoeLayer
from .competesmoe import CompeteSMoE
from .deepseek import DeepSeekV2, DeepSeekV3
from .smoe_perturbed import MoEPerturbedCosingGating, Selection
from .xmoe import XMOE
from .smoe_sigmoid import SMoEUTNorm
from .block import MoEBlock
from .smoe_ep import EPSMoeLayer
from .competesmoe_ep import EPCompeteSMoE
from .deepseek_ep import EPDeepSeekV2, EPDeepSeekV3

__all__ = ["register_moe", "get_moe", "MOE_REGISTRY", "LoggingLayer", "RegularizedLayer", "OncePerIterLayer", "CVMMSel", "cvmm",
           "cvmm_prepare_sel2", "MoE", "SMoeLayer", "CompeteSMoE", "DeepSeekV2", "DeepSeekV3", "MoEPerturbedCosingGating", "Selection", "XMOE", "SMoEUTNorm", "MoEBlock", "EPSMoeLayer",
           "EPCompeteSMoE", "EPDeepSeekV2", "EPDeepSeekV3"]

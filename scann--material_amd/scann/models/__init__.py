from .latent_index import LatentClassHead, LatentClustering, LatentEmbedding, LatentHead, LatentHierarchy, LatentIndex, LatentKernelHead, LatentPeaks, LatentProjection, LatentPrototypes
from .model_set import Ensemble, ModelSet
from .scann_model import SCANN, HipModel, create_model, create_model_pretrained, load_model, normalize_config

__all__ = ["SCANN", "HipModel", "create_model", "create_model_pretrained", "load_model", "normalize_config", "ModelSet", "Ensemble", "LatentIndex", "LatentClustering", "LatentProjection", "LatentHead", "LatentKernelHead", "LatentClassHead", "LatentEmbedding", "LatentPeaks", "LatentHierarchy", "LatentPrototypes"]

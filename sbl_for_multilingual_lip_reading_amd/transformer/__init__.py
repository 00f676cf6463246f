from .classifier import ClassifierTransformer, cal_cls_loss, cls_accuracy

__all__ = ["ClassifierTransformer", "cal_cls_loss", "cls_accuracy"]

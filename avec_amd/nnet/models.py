"""Generic model heads (nnet/models.py): the Classifier base GPT derives from, as far as GPT needs it."""
from .model import Model


class Classifier(Model):
    """nnet/models.py:24-44"""

    def __init__(self, name="Classifier"):
        super().__init__(name=name)

    def compile(self, losses=None, loss_weights=None, optimizer="Adam", metrics=None, decoders=None):
        from . import losses as L
        from . import metrics as M
        super().compile(losses=L.SoftmaxCrossEntropy() if losses is None else losses, loss_weights=loss_weights, optimizer=optimizer,
                        metrics=M.CategoricalAccuracy() if metrics is None else metrics, decoders=decoders)


model_dict = {"Classifier": Classifier}

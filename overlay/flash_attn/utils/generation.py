from hyena_dna_amd.inference import InferenceParams  # noqa: F401
from hyena_dna_amd.lm import GenerationMixin  # noqa: F401

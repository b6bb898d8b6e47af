"""Audio models: Wav2Vec2 / HuBERT, data2vec-audio, SEW and the EnCodec codec, plus the CTC heads of the
wav2vec2 family (Wav2Vec2CTC: beyond the reference).  Same import paths and class
names as the reference's pytorch_models/audio/__init__.py."""
from .ctc import Wav2Vec2CTC
from .data2vec_audio import Data2VecAudio
from .encodec import EnCodec, EnCodecDecoder, EnCodecEncoder
from .sew import SEW
from .wav2vec2 import Wav2Vec2

__all__ = ["Data2VecAudio", "EnCodec", "EnCodecDecoder", "EnCodecEncoder", "SEW", "Wav2Vec2", "Wav2Vec2CTC"]

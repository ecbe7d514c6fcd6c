"""BUILD-CONTAINER ONLY: import the reference's GPT (gpt2_model.py) and the three array helpers of its decoder.py from /root/reference, without
``transformers``, ``bark`` or ``encodec``: gpt2_model.py needs only torch and the reference's logger; decoder.py's other imports (bark, encodec, the
configs and utils modules, which download at import) are empty stand-ins, since the helpers use none of them. Nothing from the reference is copied
into this repository; only numeric outputs are saved."""
import importlib.util
import sys
import types

REF = "/root/reference/audiotoken"


class _Anything:
    def __call__(self, *a, **k):
        return self

    def __getattr__(self, name):
        return self


def _load(name):
    spec = importlib.util.spec_from_file_location(f"audiotoken.{name}", f"{REF}/{name}.py")
    m = importlib.util.module_from_spec(spec)
    sys.modules[f"audiotoken.{name}"] = m
    spec.loader.exec_module(m)
    return m


def load_reference_gpt():
    """{"gpt2_model": module, "decoder": module} under a synthetic ``audiotoken`` parent package (audiotoken/__init__.py does not run)."""
    saved = {k: sys.modules.get(k) for k in ("audiotoken", "bark", "encodec", "audiotoken.configs", "audiotoken.utils")}
    pkg = types.ModuleType("audiotoken")
    pkg.__path__ = [REF]
    sys.modules["audiotoken"] = pkg
    _load("logger")
    mods = {"gpt2_model": _load("gpt2_model")}
    anything = _Anything()   # the decoder classes' default arguments call the configs and read COMMONS.EN where the classes are defined
    stand_ins = {"bark": {}, "encodec": {"EncodecModel": anything},
                 "audiotoken.configs": {n: anything for n in ("AcousticDecoderConfig", "HubertDecoderConfig", "Wav2VecBertDecoderConfig", "COMMONS")},
                 "audiotoken.utils": {"ctx": anything}}
    for name, attrs in stand_ins.items():
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
    mods["decoder"] = _load("decoder")
    for k, v in saved.items():   # later loaders (_ref_loader) bring the real modules
        if v is None:
            sys.modules.pop(k, None)
        else:
            sys.modules[k] = v
    return mods

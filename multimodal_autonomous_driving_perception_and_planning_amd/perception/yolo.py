"""YOLO-mode model for ObjectDetector (mode="yolo"): YOLOv8 Detect models of scales n, s and m with 1 .. 256 classes on the library's
MFMA conv path (default: scale n, 80 classes).

The reference calls ultralytics `YOLO(model_path)(frame)` on whatever checkpoint it is given, "yolov8n.pt" by default
(detector.py:77-84,103-123); neither the package nor the weight file can be shipped, so this model takes its parameters from
  * a YOLOv8 `state_dict` file with ultralytics' key names (`model.0.conv.weight`, `model.0.bn.running_mean`, ...,
    `model.22.cv3.2.2.bias`), which decides scale and class count itself (infer_model): `.pt` / `.pth` / `.bin` read with `torch.load(weights_only=True)`, `.safetensors`, or an
    `.npz` of such arrays -- `torch.save(YOLO("yolov8n.pt").model.state_dict(), "yolov8n_sd.pt")` on a machine with
    ultralytics produces one (the pickled `DetectionModel` inside `yolov8n.pt` itself needs that package to load),
  * a `.npy` / `.npz` file holding the flat float32 vector in the order of `conv_specs(scale, nc)`, or
  * the pseudo path "random[:<seed>[:<scale>[:<nc>]]]" -> seeded He-normal weights with non-trivial BatchNorm
    statistics (BASELINE config 3: "random-init nano backbone").
Any other path that does not exist raises FileNotFoundError, which ObjectDetector turns into the
reference's graceful fallback to simulated mode.

Parameter order: for every convolution of conv_specs(), weight[cout][cin][k][k] followed by BatchNorm
(gamma, beta, running_mean, running_var) -- or by the bias for the two plain Conv2d that end each head branch.
"""
import ctypes as C
import os

import numpy as np
import torch

from .. import _native as nat
from .._dev import Dev

NC, REG_MAX = 80, 16
CONF_THRES, IOU_THRES, MAX_DET = 0.25, 0.7, 300          # ultralytics predict defaults

COCO_NAMES = ("person bicycle car motorcycle airplane bus train truck boat traffic_light fire_hydrant stop_sign "
              "parking_meter bench bird cat dog horse sheep cow elephant bear zebra giraffe backpack umbrella handbag "
              "tie suitcase frisbee skis snowboard sports_ball kite baseball_bat baseball_glove skateboard surfboard "
              "tennis_racket bottle wine_glass cup fork knife spoon bowl banana apple sandwich orange broccoli carrot "
              "hot_dog pizza donut cake chair couch potted_plant bed dining_table toilet tv laptop mouse remote "
              "keyboard cell_phone microwave oven toaster sink refrigerator book clock vase scissors teddy_bear "
              "hair_drier toothbrush").split()


def _c2f(c1, c2, n):
    c = c2 // 2
    return [(c1, 2 * c, 1, 1, True)] + [(c, c, 3, 1, True)] * (2 * n) + [((2 + n) * c, c2, 1, 1, True)]


# yolov8.yaml `scales`: depth, width, max_channels.  n, s and m are built; l and x are known so that they can be refused by name.
SCALES = {"n": (0.33, 0.25, 1024), "s": (0.33, 0.50, 1024), "m": (0.67, 0.75, 768), "l": (1.00, 1.00, 512), "x": (1.00, 1.25, 512)}
BUILT_SCALES = ("n", "s", "m")
MAX_NC = 256


def _check_model(scale, nc):
    if scale not in SCALES:
        raise ValueError("unknown YOLOv8 scale %r (n, s and m are built)" % (scale,))
    if scale not in BUILT_SCALES:
        raise ValueError("YOLOv8 scale %r is not built (n, s and m are)" % (scale,))
    if not (isinstance(nc, (int, np.integer)) and 1 <= nc <= MAX_NC):
        raise ValueError("nc = %r: 1 .. %d classes are built" % (nc, MAX_NC))


def model_dims(scale="n", nc=NC):
    """yolov8.yaml's rules for one scale: -> (stage widths c1..c5, C2f repeats of layers 2/4/6/8, repeats of the neck's C2f blocks,
    hidden width of Detect's box branch, hidden width of its class branch).  Channels are make_divisible(min(c, max_channels) width,
    8), repeats max(round(n depth), 1).  Any scale of SCALES (infer_model recognises l and x by these numbers)."""
    depth, width, max_ch = SCALES[scale]
    ch = tuple(int(-(-min(c, max_ch) * width // 8)) * 8 for c in (64, 128, 256, 512, 1024))
    rep = tuple(max(round(n * depth), 1) for n in (3, 6, 6, 3))
    return ch, rep, max(round(3 * depth), 1), max(16, ch[2] // 4, 4 * REG_MAX), max(ch[2], min(nc, 100))


def native_model(scale="n", nc=NC):
    """The library's av_yolo_model for (scale, nc) (av_yolo_model_preset)."""
    m = nat.YoloModel()
    nat.check(nat.lib().av_yolo_model_preset(ord(scale) if len(scale) == 1 else 0, int(nc), C.byref(m)))
    return m


def conv_specs(scale="n", nc=NC):
    """[(cin, cout, k, stride, has_bn_act)] in execution order (yolov8.yaml)."""
    _check_model(scale, nc)
    (c1, c2, c3, c4, c5), rep, nr, hb, hc = model_dims(scale, nc)
    s = [(3, c1, 3, 2, True), (c1, c2, 3, 2, True)] + _c2f(c2, c2, rep[0])
    s += [(c2, c3, 3, 2, True)] + _c2f(c3, c3, rep[1]) + [(c3, c4, 3, 2, True)] + _c2f(c4, c4, rep[2])
    s += [(c4, c5, 3, 2, True)] + _c2f(c5, c5, rep[3]) + [(c5, c5 // 2, 1, 1, True), (2 * c5, c5, 1, 1, True)]
    s += _c2f(c5 + c4, c4, nr) + _c2f(c4 + c3, c3, nr) + [(c3, c3, 3, 2, True)] + _c2f(c3 + c4, c4, nr)
    s += [(c4, c4, 3, 2, True)] + _c2f(c4 + c5, c5, nr)
    for ch in (c3, c4, c5):
        s += [(ch, hb, 3, 1, True), (hb, hb, 3, 1, True), (hb, 4 * REG_MAX, 1, 1, False)]
        s += [(ch, hc, 3, 1, True), (hc, hc, 3, 1, True), (hc, nc, 1, 1, False)]
    return s


def param_count(scale="n", nc=NC):
    """Floats in the flat vector of conv_specs(scale, nc)."""
    return sum(cout * cin * k * k + (4 if bn else 1) * cout for cin, cout, k, _, bn in conv_specs(scale, nc))


def trainable_count(scale="n", nc=NC):
    """The figure ultralytics prints: weights + two per BatchNorm channel + biases + the 16 constant DFL weights."""
    return sum(cout * cin * k * k + (2 if bn else 1) * cout for cin, cout, k, _, bn in conv_specs(scale, nc)) + REG_MAX


def random_params(seed=0, scale="n", nc=NC):
    rs = np.random.RandomState(seed)
    parts = []
    for cin, cout, k, _, bn in conv_specs(scale, nc):
        parts.append((rs.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32).ravel())
        if bn:
            parts += [rs.uniform(0.8, 1.2, cout).astype(np.float32), rs.uniform(-0.1, 0.1, cout).astype(np.float32),
                      rs.uniform(-0.1, 0.1, cout).astype(np.float32), rs.uniform(0.8, 1.2, cout).astype(np.float32)]
        else:
            parts.append(rs.uniform(-1.0, 1.0, cout).astype(np.float32))
    return np.concatenate(parts)


def ultralytics_layer_names(scale="n"):
    """The module path of every convolution of conv_specs(scale), in that order, in ultralytics' YOLOv8 `state_dict`
    (`model.<layer>.…`; a Conv block holds `.conv.weight` + `.bn.{weight,bias,running_mean,running_var}`, the two plain
    Conv2d that end a Detect branch hold `.weight` + `.bias`) -- yolov8.yaml layer numbers, nn/modules/{conv,block,head}.py:
    C2f = cv1, m.<i>.cv1, m.<i>.cv2, cv2; SPPF = cv1, cv2; Detect = cv2.<level>.<0..2> (box), cv3.<level>.<0..2> (class)."""
    _check_model(scale, NC)
    _, rep, nr, _, _ = model_dims(scale)

    def c2f(layer, n):
        return (["%d.cv1" % layer] + [q for i in range(n) for q in ("%d.m.%d.cv1" % (layer, i), "%d.m.%d.cv2" % (layer, i))]
                + ["%d.cv2" % layer])
    names = ["0", "1"] + c2f(2, rep[0]) + ["3"] + c2f(4, rep[1]) + ["5"] + c2f(6, rep[2]) + ["7"] + c2f(8, rep[3]) + ["9.cv1", "9.cv2"]
    names += c2f(12, nr) + c2f(15, nr) + ["16"] + c2f(18, nr) + ["19"] + c2f(21, nr)
    for lvl in range(3):
        names += ["22.cv2.%d.%d" % (lvl, j) for j in range(3)] + ["22.cv3.%d.%d" % (lvl, j) for j in range(3)]
    return names


def _strip_prefixes(sd):
    import re
    return {re.sub(r"^(?:(?:model|module)\.)+", "", k): v for k, v in sd.items()}


def infer_model(sd):
    """(scale, nc) of a YOLOv8 Detect `state_dict`, read from its shapes: the rows of `0.conv.weight` (16 / 32 / 48 / 64 / 80 for n / s /
    m / l / x), the `m.<i>` bottlenecks of layer 2 (they must be the scale's repeat count) and the rows of `22.cv3.0.2.weight` (nc).
    ValueError naming the scale for l and x, which are not built; ValueError naming the key for anything that is not such a model."""
    flat = _strip_prefixes(sd)

    def rows(key):
        if key not in flat:
            raise ValueError("state_dict has no %r: not a YOLOv8 Detect model's state_dict" % ("model." + key))
        shape = tuple(flat[key].shape)
        if len(shape) != 4:
            raise ValueError("%s has shape %s: not a YOLOv8 Detect model's state_dict" % ("model." + key, shape))
        return shape[0]
    c1 = rows("0.conv.weight")
    by_width = {model_dims(s)[0][0]: s for s in SCALES}
    if c1 not in by_width:
        raise ValueError("model.0.conv.weight has %d rows: no YOLOv8 scale starts with that width (%s)" % (
            c1, ", ".join("%s: %d" % (s, w) for w, s in sorted(by_width.items()))))
    scale = by_width[c1]
    reps = len({k.split(".")[2] for k in flat if k.startswith("2.m.") and k.endswith(".cv1.conv.weight")})
    if reps != model_dims(scale)[1][0]:
        raise ValueError("layer 2 has %d bottlenecks under model.2.m.<i>, YOLOv8%s has %d" % (reps, scale, model_dims(scale)[1][0]))
    nc = rows("22.cv3.0.2.weight")
    if scale not in BUILT_SCALES:
        raise ValueError("a YOLOv8%s state_dict (scale %r, %d classes): scales n, s and m are built, l and x are not" % (scale, scale, nc))
    _check_model(scale, nc)
    return scale, nc


def params_from_state_dict(sd, scale=None, nc=None):
    """Flat parameter vector (the order of conv_specs()) from a YOLOv8 `state_dict` with ultralytics' key names
    (detector.py:77-84 loads such a model through `YOLO(model_path)`).  The dict decides scale and nc itself (infer_model); given
    arguments must agree with it.  Keys may carry any number of leading `model.` / `module.` prefixes; `num_batches_tracked` and the
    constant DFL convolution (`22.dfl.conv.weight`, arange(16)) are ignored; every shape is checked.  BatchNorm is folded later by the
    library (eps 1e-3, ultralytics' Conv default)."""
    flat = _strip_prefixes(sd)
    found = infer_model(flat)
    if (scale is not None and scale != found[0]) or (nc is not None and nc != found[1]):
        raise ValueError("the state_dict is a YOLOv8%s with %d classes, scale=%r nc=%r was asked for" % (found + (scale, nc)))
    scale, nc = found
    specs, names = conv_specs(scale, nc), ultralytics_layer_names(scale)
    assert len(specs) == len(names)

    def get(key, shape):
        if key not in flat:
            raise KeyError("state_dict has no %r (a YOLOv8%s checkpoint's state_dict is expected)" % ("model." + key, scale))
        a = flat[key]
        a = a.detach().cpu().float().numpy() if hasattr(a, "detach") else np.asarray(a, np.float32)
        if tuple(a.shape) != tuple(shape):
            raise ValueError("%s has shape %s, YOLOv8%s (scale %s, %d classes) needs %s" % (key, tuple(a.shape), scale, scale, nc, tuple(shape)))
        return np.ascontiguousarray(a, np.float32).ravel()
    parts = []
    for (cin, cout, k, _, bn), name in zip(specs, names):
        if bn:
            parts.append(get(name + ".conv.weight", (cout, cin, k, k)))
            parts += [get(name + ".bn." + q, (cout,)) for q in ("weight", "bias", "running_mean", "running_var")]
        else:
            parts += [get(name + ".weight", (cout, cin, k, k)), get(name + ".bias", (cout,))]
    return np.concatenate(parts)


def model_of_params(params, scale=None, nc=None):
    """(scale, nc) for a flat vector: the arguments (defaults n, 80), checked against the vector's length."""
    scale, nc = scale or "n", NC if nc is None else nc
    n = param_count(scale, nc)
    if np.size(params) != n:
        raise ValueError("parameter vector has %d floats, the YOLOv8%s graph with %d classes needs %d" % (np.size(params), scale, nc, n))
    return scale, nc


def state_dict_from_params(params, prefix="model.", scale=None, nc=None):
    """Inverse of params_from_state_dict (NumPy arrays under ultralytics' key names): lets a parameter vector of this
    project be handed to code that expects a YOLOv8 state_dict, and is what the round-trip test uses."""
    params = np.asarray(params, np.float32).ravel()
    scale, nc = model_of_params(params, scale, nc)
    sd, pos = {}, 0
    for (cin, cout, k, _, bn), name in zip(conv_specs(scale, nc), ultralytics_layer_names(scale)):
        nw = cout * cin * k * k
        w = params[pos:pos + nw].reshape(cout, cin, k, k)
        pos += nw
        if bn:
            sd[prefix + name + ".conv.weight"] = w
            for q in ("weight", "bias", "running_mean", "running_var"):
                sd[prefix + name + ".bn." + q] = params[pos:pos + cout]
                pos += cout
        else:
            sd[prefix + name + ".weight"] = w
            sd[prefix + name + ".bias"] = params[pos:pos + cout]
            pos += cout
    assert pos == params.size
    return sd


def _load_checkpoint(model_path):
    """A torch file (`.pt` / `.pth` / `.bin`) or `.safetensors` -> state_dict.  Only plain tensor containers are read
    (`weights_only=True`): a state_dict, or a dict holding one under "state_dict" / "model_state_dict" / "model".  An
    ultralytics training checkpoint pickles the whole `DetectionModel` object, which cannot be rebuilt without that package --
    save `YOLO("yolov8n.pt").model.state_dict()` once instead."""
    if model_path.endswith(".safetensors"):
        from safetensors.numpy import load_file
        return load_file(model_path)
    try:
        obj = torch.load(model_path, map_location="cpu", weights_only=True)
    except Exception as e:                                  # pickled module classes (ultralytics.nn.tasks.DetectionModel, ...)
        raise FileNotFoundError("%r is not a plain state_dict file (%s: %s); export one with "
                                "torch.save(YOLO(path).model.state_dict(), out)" % (model_path, type(e).__name__, str(e)[:120]))
    names = obj.get("names") if isinstance(obj, dict) else None
    for key in ("state_dict", "model_state_dict", "model"):
        if isinstance(obj, dict) and isinstance(obj.get(key), dict):
            obj = obj[key]
            names = obj.get("names", names)
    if not isinstance(obj, dict):
        raise FileNotFoundError("%r holds a %s, not a state_dict" % (model_path, type(obj).__name__))
    if isinstance(names, (list, tuple, dict)):              # a checkpoint's class names ride along under a key no layer has
        obj = dict(obj, names=names)
    return obj


def _names_dict(names, nc, what):
    """{class id: name} from a list or a dict with the ids 0 .. nc-1."""
    d = {int(k): str(v) for k, v in names.items()} if isinstance(names, dict) else dict(enumerate(str(v) for v in names))
    if sorted(d) != list(range(nc)):
        raise ValueError("%s name %d classes, the model has %d" % (what, len(d), nc))
    return d


def load_model(model_path, scale=None, nc=None):
    """-> (flat parameter vector, scale, nc, names or None).  A state_dict decides scale and nc itself and given arguments must agree
    with it; "random[:seed[:scale[:nc]]]" and flat vectors take the arguments (the path's fields first; defaults n, 80) and the
    vector's length is checked; a NumPy array in place of the path is taken as the flat vector.  names: the `names` entry of a checkpoint dict (list or dict, which weights_only=True loads) or of an
    .npz state_dict (an array of strings), else None."""
    def from_sd(sd):
        sd = dict(sd)
        names = sd.pop("names", None)
        p = params_from_state_dict(sd, scale, nc)
        return (p,) + infer_model(sd) + (names,)

    def from_vector(p, scale, nc):
        p = np.ascontiguousarray(p, np.float32).ravel()
        return (p,) + model_of_params(p, scale, nc) + (None,)
    if isinstance(model_path, np.ndarray):                  # the flat vector itself
        return from_vector(model_path, scale, nc)
    if model_path.startswith("random"):
        f = model_path.split(":")
        seed = int(f[1]) if len(f) > 1 and f[1] else 0
        p_scale, p_nc = (f[2] if len(f) > 2 else None), (int(f[3]) if len(f) > 3 else None)
        if (scale is not None and p_scale is not None and scale != p_scale) or (nc is not None and p_nc is not None and nc != p_nc):
            raise ValueError("%r and scale=%r, nc=%r disagree" % (model_path, scale, nc))
        scale, nc = p_scale or scale or "n", p_nc if p_nc is not None else (NC if nc is None else nc)
        return random_params(seed, scale, nc), scale, nc, None
    if not os.path.exists(model_path):
        raise FileNotFoundError("model file %r not found (pass a YOLOv8 n/s/m state_dict file (.pt/.pth/.safetensors), a "
                                ".npy/.npz parameter vector or 'random[:seed[:scale[:nc]]]')" % model_path)
    if model_path.endswith(".npz"):
        z = np.load(model_path)
        if len(z.files) > 1:                                # a state_dict saved with np.savez
            sd = {k: z[k] for k in z.files}
            if "names" in sd:
                sd["names"] = [str(v) for v in sd["names"]]
            return from_sd(sd)
        return from_vector(z[z.files[0]], scale, nc)
    if model_path.endswith(".npy"):
        return from_vector(np.load(model_path), scale, nc)
    return from_sd(_load_checkpoint(model_path))


def load_params(model_path, scale=None, nc=None):
    return load_model(model_path, scale, nc)[0]


class _OwnStream:
    """A Dev with a stream of its own (stream capture needs a non-default stream; the per-frame detector call keeps its upload,
    its graph replay and its wait on it)."""

    def __init__(self, dev):
        self.index, self.device, self.ctx, self.lib = dev.index, dev.device, dev.ctx, dev.lib
        self._stream = torch.cuda.Stream(device=dev.device)

    @property
    def stream(self):
        return nat.stream_handle(self._stream)

    def sync(self):
        self._stream.synchronize()


class YoloV8:
    def __init__(self, model_path="random", device=0, batch=1, keep_logits=False, precision="fp16", scale=None, nc=None, names=None):
        """scale ("n", "s", "m"), nc (1 .. 256): the model, for "random[:seed[:scale[:nc]]]" and flat vectors (defaults n, 80); a
        state_dict decides both itself and the arguments, if given, must agree.  names: class names (a list, or a dict by class id);
        default: the checkpoint's `names` entry, else COCO's for 80 classes, else {i: "class<i>"}.
        keep_logits: test hook -- the head also writes its float32 logits (tensor ids 100-105) and the stand-alone decode
        runs on them (ids 120-122); normally the decode happens in the head's last convolutions and no logits exist.
        precision: "fp16" -- IEEE-half tensors / weights / MFMA operands with float32 accumulation, the fused production path;
        "fp32" -- the reference's own arithmetic (ultralytics on torch float32, detector.py:103-123): float32 everywhere on
        v_mfma_f32_16x16x4_f32, one generic kernel per layer, logits always kept (ids 100-105)."""
        if precision not in ("fp16", "fp32"):
            raise ValueError("precision must be 'fp16' or 'fp32', got %r" % (precision,))
        self._dev = Dev(device)
        self.keep_logits = keep_logits
        self.params, self.scale, self.nc, file_names = load_model(model_path, scale, nc)
        self._model = native_model(self.scale, self.nc)
        n = int(self._dev.lib.av_yolo_model_param_count(C.byref(self._model)))
        if self.params.size != n:
            raise ValueError("parameter vector has %d floats, the YOLOv8%s graph with %d classes needs %d" % (self.params.size, self.scale, self.nc, n))
        if names is not None:
            self.names = _names_dict(names, self.nc, "names")
        elif file_names is not None:
            self.names = _names_dict(file_names, self.nc, "the checkpoint's names")
        else:
            self.names = dict(enumerate(COCO_NAMES)) if self.nc == NC else {i: "class%d" % i for i in range(self.nc)}
        self.batch = batch
        self.precision = precision
        self._h = None
        self._shape = None
        self._io_in = self._io_out = None      # per-frame call: pinned upload buffer, host-mapped result buffer
        self._io_shape = None
        # per-frame call (batch 1): the whole forward -- ~56 launches on two lanes -- is captured into ONE hipGraph after the first
        # eager call and replayed from then on (demo.py:107 calls the detector once per frame: launch overhead, not kernel time,
        # is what a single 384x640 image costs).  AVHOT_YOLO_NO_GRAPH=1 keeps the eager launches.
        self._gdev = None
        self._graphs = {}                      # (conf, iou) -> graph id, for the current shape
        self._warm = set()
        self.use_graph = os.environ.get("AVHOT_YOLO_NO_GRAPH", "0") != "1"

    def _prepare(self, h, w):
        if self._shape == (h, w):
            return
        d = self._dev
        self.close()
        hd = C.c_void_p()
        nat.check(d.lib.av_yolo_create_model(d.ctx.handle, self.batch, h, w, C.byref(self._model), self.params.ctypes.data_as(C.c_void_p),
                                             self.params.size, 1 if self.precision == "fp32" else 0, C.byref(hd)))
        self._h = hd
        self._shape = (h, w)
        if self.keep_logits:
            nat.check(d.lib.av_yolo_keep_logits(hd, 1))
        B = self.batch
        self._frames = d.empty((B, h, w, 3), torch.uint8)
        self._n = d.zeros(B, torch.int32)
        self._box = d.zeros((B, MAX_DET, 4), torch.float32)
        self._conf = d.zeros((B, MAX_DET), torch.float32)
        self._cls = d.zeros((B, MAX_DET), torch.int32)

    def dims(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        nat.check(self._dev.lib.av_yolo_dims(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def forward_device(self, frames_dev, conf=CONF_THRES, iou=IOU_THRES):
        """frames_dev: uint8 [batch, h, w, 3] device tensor.  Enqueues the whole detector; results stay on device."""
        d = self._dev
        nat.check(d.lib.av_yolo_forward(self._h, d.stream, nat.ptr(frames_dev), conf, iou, MAX_DET, nat.ptr(self._n),
                                        nat.ptr(self._box), nat.ptr(self._conf), nat.ptr(self._cls)))

    def detect(self, frame, conf=CONF_THRES, iou=IOU_THRES):
        """One BGR frame -> (boxes float32[n,4] xyxy in frame pixels, conf[n], cls[n]).  The per-frame call of the drop-in
        class: the frame goes up through one pinned buffer (host copy and DMA pipelined in pieces), the detections come back
        through one host-mapped buffer the NMS kernel writes directly (no copy commands, no .item(): one polling wait)."""
        frame = np.ascontiguousarray(frame, np.uint8)
        h, w = frame.shape[:2]
        self._prepare(h, w)
        if self.batch != 1:
            self._frames[0].copy_(torch.as_tensor(frame))
            self.forward_device(self._frames, conf, iou)
            n = int(self._n[0].item())
            return (self._box[0, :n].cpu().numpy(), self._conf[0, :n].cpu().numpy(), self._cls[0, :n].cpu().numpy())
        if self._gdev is None:
            self._gdev = _OwnStream(self._dev)
        d = self._gdev
        if self._io_shape != (h, w):
            from .._dev import Packed
            for io in (self._io_in, self._io_out):
                if io is not None:
                    io.close()
            self._io_in = Packed(d, [("frame", np.uint8, (h, w, 3))], mapped=False)
            self._io_out = Packed(d, [("n", np.int32, (1,)), ("box", np.float32, (MAX_DET, 4)), ("conf", np.float32, (MAX_DET,)),
                                      ("cls", np.int32, (MAX_DET,))], mapped=True)
            self._io_shape = (h, w)
        self._io_in.upload_from("frame", frame)
        o = self._io_out

        def enqueue():
            nat.check(d.lib.av_yolo_forward(self._h, d.stream, self._io_in.ptr("frame"), conf, iou, MAX_DET, o.ptr("n"), o.ptr("box"),
                                            o.ptr("conf"), o.ptr("cls")))
        key = (float(conf), float(iou))
        gid = self._graphs.get(key)
        if gid is None and self.use_graph and key in self._warm and not self.keep_logits and self.precision == "fp16":
            # second call with these thresholds: every one-time host action of the forward (symbol uploads, attributes) is behind us
            g = C.c_int(-1)
            nat.check(d.lib.av_graph_begin(d.ctx.handle, d.stream))
            try:
                enqueue()
            finally:
                nat.check(d.lib.av_graph_end(d.ctx.handle, d.stream, C.byref(g)))
            gid = self._graphs[key] = g.value
        if gid is not None:
            nat.check(d.lib.av_graph_launch(d.ctx.handle, gid, d.stream))
        else:
            enqueue()
            self._warm.add(key)
        o.download()
        n = int(o.h["n"][0])
        return o.h["box"][:n].copy(), o.h["conf"][:n].copy(), o.h["cls"][:n].copy()

    def tensor(self, tid, image=0):
        """Host copy (float32, [H, W, C]) of an intermediate tensor of one image of the batch, or of all images
        ([batch, H, W, C]) with image=None (test hook)."""
        p, H, W, Cc, cs, co = C.c_void_p(), C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        nat.check(self._dev.lib.av_yolo_tensor(self._h, tid, C.byref(p), C.byref(H), C.byref(W), C.byref(Cc), C.byref(cs),
                                               C.byref(co)))
        if 100 <= tid < 106 and not (self.keep_logits or self.precision == "fp32"):
            raise RuntimeError("head logits exist only in a YoloV8n(keep_logits=True) or in float32 mode")
        n = self.batch * H.value * W.value * cs.value
        t = torch.empty(n, dtype=torch.float32 if (tid >= 100 or self.precision == "fp32") else torch.int16, device=self._dev.device)
        nbytes = t.numel() * t.element_size()
        self._dev.sync()
        rc = _memcpy_d2d(t.data_ptr(), p.value, nbytes)      # the tensor lives in library-owned memory
        if rc != 0:
            raise RuntimeError("hipMemcpy failed (%d)" % rc)
        arr = t.cpu().numpy().reshape(self.batch, H.value, W.value, cs.value)[..., co.value:co.value + Cc.value]
        if image is not None:
            arr = arr[image]
        if tid in (112, 122):
            return np.ascontiguousarray(arr).view(np.int32)
        if tid >= 100 or self.precision == "fp32":
            return arr.astype(np.float32)
        if self.precision == "bf16":                       # (a library built with bf16 activations: comparison runs only)
            return (arr.astype(np.uint16).astype(np.uint32) << 16).view(np.float32)
        return np.ascontiguousarray(arr).view(np.float16).astype(np.float32)

    def ops(self):
        """The ops of the network as the library built them, one per layer in execution order (test hook av_yolo_op): a list of
        nat.YoloOpInfo.  Reads nothing from the device."""
        n = C.c_int()
        nat.check(self._dev.lib.av_yolo_op_count(self._h, C.byref(n)))
        out = []
        for k in range(n.value):
            info = nat.YoloOpInfo()
            nat.check(self._dev.lib.av_yolo_op(self._h, k, C.byref(info)))
            out.append(info)
        return out

    def tail(self, box, conf, cls, conf_thres=CONF_THRES, iou_thres=IOU_THRES, max_det=MAX_DET, out=None):
        """The forward's threshold + sort + NMS + scale_boxes on given candidates (test hook av_yolo_tail): box float32 [batch, A, 4] in
        network pixels, conf float32 [batch, A], cls int32 [batch, A] (A = dims()[2]), as arrays or device tensors.  out: the device
        tensors (n int32 [batch], box float32 [batch, max_det, 4], conf float32 [batch, max_det], cls int32 [batch, max_det]) the
        library writes; default: fresh ones filled with zeros.  -> host copies of the four; rows at and beyond n[b] are not written."""
        d, A = self._dev, self.dims()[2]

        def up(a, dtype, shape):
            np_dtype = np.float32 if dtype == torch.float32 else np.int32
            t = a if torch.is_tensor(a) else torch.as_tensor(np.array(a, np_dtype))    # (a writable copy: as_tensor refuses read-only arrays)
            t = t.to(d.device).contiguous()
            if t.dtype != dtype or tuple(t.shape) != shape:
                raise ValueError("candidates must be %s %s, got %s %s" % (dtype, shape, t.dtype, tuple(t.shape)))
            return t
        B = self.batch
        cb, cc, ck = up(box, torch.float32, (B, A, 4)), up(conf, torch.float32, (B, A)), up(cls, torch.int32, (B, A))
        if out is None:
            out = (d.zeros(B, torch.int32), d.zeros((B, max_det, 4), torch.float32), d.zeros((B, max_det), torch.float32),
                   d.zeros((B, max_det), torch.int32))
        nat.check(d.lib.av_yolo_tail(self._h, d.stream, nat.ptr(cb), nat.ptr(cc), nat.ptr(ck), conf_thres, iou_thres, int(max_det),
                                     *[nat.ptr(t) for t in out]))
        d.sync()
        return tuple(t.cpu().numpy() for t in out)

    def plan(self):
        """The launches of a forward as they are planned now, in order (test hook av_yolo_plan_step): a list of nat.YoloStepInfo.
        Reads nothing from the device."""
        n = C.c_int()
        nat.check(self._dev.lib.av_yolo_plan_count(self._h, C.byref(n)))
        out = []
        for k in range(n.value):
            info = nat.YoloStepInfo()
            nat.check(self._dev.lib.av_yolo_plan_step(self._h, k, C.byref(info)))
            out.append(info)
        return out

    def _read(self, ptr, count, dtype):
        """Host copy of `count` elements of library-owned device memory."""
        t = torch.empty(count, dtype=dtype, device=self._dev.device)
        self._dev.sync()
        rc = _memcpy_d2d(t.data_ptr(), ptr, t.numel() * t.element_size())
        if rc != 0:
            raise RuntimeError("hipMemcpy failed (%d)" % rc)
        return t.cpu().numpy()

    def read_slice(self, s):
        """Host copy of a nat.YoloSlice of an op, all images: float32 or float16 [batch, H, W, c] (test hook)."""
        a = self._read(s.ptr, self.batch * s.H * s.W * s.cstride, torch.float32 if s.f32 else torch.float16)
        return np.ascontiguousarray(a.reshape(self.batch, s.H, s.W, s.cstride)[..., s.coff:s.coff + s.c])

    def read_weights(self, op):
        """Host copy of a convolution op's folded weights, float32 or float16 [cout, kpad], and of its float32 bias [cout] (test hook)."""
        w = self._read(op.wgt, op.cout * op.kpad, torch.float32 if op.wgt_f32 else torch.float16).reshape(op.cout, op.kpad)
        return w, self._read(op.bias, op.cout, torch.float32)

    def close(self):
        if self._h is not None:
            self._dev.sync()
            if self._gdev is not None:
                self._gdev.sync()
            for gid in self._graphs.values():           # the graphs hold this handle's buffers and kernel arguments
                self._dev.lib.av_graph_destroy(self._dev.ctx.handle, gid)
            self._graphs, self._warm = {}, set()
            self._dev.lib.av_yolo_destroy(self._h)
            self._h = None
        for io in (getattr(self, "_io_in", None), getattr(self, "_io_out", None)):
            if io is not None:
                io.close()
        self._io_in = self._io_out = None
        self._io_shape = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


YoloV8n = YoloV8          # the name of the default model (scale n, 80 classes)


def _memcpy_d2d(dst, src, nbytes):
    import ctypes
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return hip.hipMemcpy(dst, src, nbytes, 3)      # hipMemcpyDeviceToDevice

"""FastAPI service: create / import / train / evaluate / generate / diagnose models.

Route and schema parity with the reference service (``main.py:21-506``): ``/``, ``/dashboard``,
``/static``, ``POST /model/``, ``POST /import/``, ``GET|POST|DELETE /dataset/``,
``POST /tokenize/``, ``POST /output/``, ``POST /evaluate/``, ``POST /generate/`` (JSON or
``text/plain`` token stream), ``POST /decode/``, ``PUT /train/``, ``GET /progress/``,
``GET /stats/``, ``DELETE /model/``; gzip request bodies; ``KeyError``→404, ``ValueError``→400,
other exceptions→500; per-id locks (409 while a job holds them).

MI355X-first differences:
  * serving runs on the GPU (``PENROZ_SERVE_DEVICE``, default ``cuda`` when present) with a small
    model cache keyed on the checkpoint's mtime, instead of rebuilding the model on the CPU for
    every request (``/generate`` uses the preallocated KV cache + decode-attention kernel);
  * ``/train/`` runs the launcher (one worker per GPU, RCCL) and checks its exit code: a failed
    run marks the model ``Error`` instead of leaving it ``Training`` (reference bug 9);
    ``max_grad_norm`` clips the gradients by global norm (``ops/grad_clip.py``; invalid values
    are a 400 before any worker starts) and adds ``grad_norm`` to the progress records;
  * ``/progress/`` reads a small sidecar JSON instead of ``torch.load``-ing the checkpoint.
"""
from __future__ import annotations

import asyncio
import gzip
import logging
import math
import os
import threading
from asyncio import Lock, create_task
from typing import Dict

from fastapi import Body, FastAPI, HTTPException, Request
from fastapi.concurrency import run_in_threadpool
from fastapi.encoders import jsonable_encoder
from fastapi.exceptions import RequestValidationError
from fastapi.params import Query
from fastapi.responses import HTMLResponse, JSONResponse, RedirectResponse, Response, StreamingResponse
from fastapi.staticfiles import StaticFiles
from pydantic import BaseModel, Field, StrictInt

from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel, call_shape_of
from penroz.ops import grad_clip as grad_clip_ops
from penroz.ops import weight_quant as wq_ops
from penroz.ops.decode_options import KEYWORDS, NOT_LOADED, check_options
from penroz.parallel import launcher
from penroz.utils.loaders import Downloader, Loader
from penroz.utils.tokenizers import Tokenizer

log = logging.getLogger(__name__)

HERE = os.path.dirname(os.path.abspath(__file__))

app = FastAPI(title="penroz — MI355X neural network model API",
              description="Create, import, train, evaluate, generate with and diagnose neural network models "
                          "on AMD Instinct MI355X.",
              version="0.1.0")
app.mount("/static", StaticFiles(directory=os.path.join(HERE, "static")), name="static")

dataset_locks: Dict[str, Lock] = {}
model_locks: Dict[str, Lock] = {}


def _gpt2_example_layers(V=50304, C=768, L=12, H=12, P=1024) -> list[dict]:
    std2 = 0.02 / math.sqrt(2 * L)
    def lin(i, o, std):
        return {"linear": {"in_features": i, "out_features": o}, "normal": {"mean": 0.0, "std": std}, "zeros": {}}
    blocks = [{"residual": [
        {"sequential": [{"layernorm": {"normalized_shape": C}}, lin(C, 3 * C, 0.02),
                        {"attention": {"num_heads": H, "dropout": 0.0}}, lin(C, C, std2), {"dropout": {"p": 0.0}}]},
        {"sequential": [{"layernorm": {"normalized_shape": C}}, lin(C, 4 * C, 0.02), {"gelu": {}},
                        lin(4 * C, C, std2), {"dropout": {"p": 0.0}}]}]} for _ in range(L)]
    return ([{"summation": [{"embedding": {"num_embeddings": V, "embedding_dim": C}, "normal": {"mean": 0.0, "std": 0.02}},
                            {"position": {"num_embeddings": P, "embedding_dim": C}, "normal": {"mean": 0.0, "std": 0.02}}]},
             {"dropout": {"p": 0.0}}] + blocks +
            [{"layernorm": {"normalized_shape": C}}, {"linear": {"in_features": C, "out_features": V, "bias": False}},
             {"softmaxlast": {"dim": -1}}])


# ------------------------------------------------------------------------------ schemas
class ModelRequest(BaseModel):
    model_id: str = Field(..., examples=["gpt-example"], description="The unique identifier for the model.")


class ModelOnDeviceRequest(ModelRequest):
    device: str = Field("cpu", examples=["cpu", "cuda"], description="Device to run on (cuda = every GPU, RCCL)")


class CreateModelRequest(ModelRequest):
    layers: list[dict] = Field(..., examples=[_gpt2_example_layers()],
                               description="Layer list: each item maps an algo (and init keys) to its args.")
    optimizer: dict = Field(..., examples=[{"adamw": {"lr": 6e-4, "betas": [0.9, 0.95], "eps": 1e-8}}],
                            description="Optimizer name mapped to its args (adam, adamw, sgd).")


class DatasetRequest(BaseModel):
    dataset_id: str = Field(..., examples=["tiny-shakespeare"], description="The unique identifier for the dataset")


class TokenizerRequest(BaseModel):
    encoding: str = Field(..., examples=["tiktoken/gpt2"],
                          description="tiktoken encoding (prefix 'tiktoken/') or HuggingFace tokenizer name")


class DownloadDatasetRequest(DatasetRequest, TokenizerRequest):
    path: str = Field(..., examples=["andriotis/tiny-shakespeare-karpathy"])
    name: str = Field(..., examples=["default"])
    split: str = Field(..., examples=["train"])
    shard_size: int = Field(..., examples=[100000], description="Tokens per shard")


class BatchedRunRequest(ModelOnDeviceRequest, DatasetRequest):
    shard: int = Field(..., examples=[1], description="Dataset shard to begin from")
    epochs: int = Field(..., examples=[4], description="Number of training epochs")
    batch_size: int = Field(..., examples=[2], description="Sequences per rank per micro-step")
    block_size: int = Field(..., examples=[1024], description="Sequence length")
    step_size: int = Field(..., examples=[2], description="Sequences per accumulation step")


class TrainingRequest(BatchedRunRequest):
    # (bool listed so that ``true`` reaches the check below as a bool and gets its 400, not a silent 1.0)
    max_grad_norm: float | bool | None = Field(
        None, examples=[1.0], json_schema_extra={"anyOf": [{"type": "number", "exclusiveMinimum": 0}, {"type": "null"}]},
        description="Clip the gradients of every optimizer step by their global L2 norm "
                    "(torch.nn.utils.clip_grad_norm_): a finite number > 0; null: off. With a value, every "
                    "progress record carries grad_norm, the pre-clip norm")


class EvaluateRequest(BatchedRunRequest):
    target_dataset_id: str | None = Field(None, examples=[None], description="Separate target dataset (optional)")
    shard: int = Field(..., examples=[0])
    epochs: int = Field(..., examples=[2])
    step_size: int = Field(..., examples=[1])


class TokenizeTextRequest(TokenizerRequest):
    text: str = Field(..., examples=["PENR-OZ:\nI say Hello world!"])


class OutputRequest(ModelRequest):
    input: list = Field(..., examples=[[[0]]], description="The initial input context")
    target: list | int | None = Field(None, examples=[None], description="Expected target (optional)")


class GenerateRequest(ModelRequest):
    input: list = Field(..., examples=[[[0]]], description="The initial input context")
    block_size: int = Field(..., examples=[1024], description="Context block size")
    max_new_tokens: int = Field(..., examples=[10])
    temperature: float = Field(1.0, examples=[1.0])
    top_k: int | None = Field(None, examples=[None])
    top_p: float | None = Field(None, gt=0, le=1, examples=[None],
                                description="Nucleus sampling: keep the most likely tokens up to this probability mass")
    min_p: float | None = Field(None, ge=0, lt=1, examples=[None],
                                description="Keep tokens at least this likely relative to the most likely one")
    repetition_penalty: float | None = Field(None, gt=0, allow_inf_nan=False, examples=[None],
                                             description="Divide the positive (multiply the negative) logits of tokens "
                                                         "seen in the prompt or generated so far; 1.0: off")
    presence_penalty: float | None = Field(None, allow_inf_nan=False, examples=[None],
                                           description="Subtracted from the logit of every token generated so far")
    frequency_penalty: float | None = Field(None, allow_inf_nan=False, examples=[None],
                                            description="Subtracted from a token's logit once per time it was "
                                                        "generated")
    logprobs: int | None = Field(None, ge=0, le=20, examples=[None],
                                 description="Return each generated token's log-probability and this many most "
                                             "likely tokens with theirs (0: the chosen tokens' only); null: off")
    stop_token: int | None = Field(None, examples=[None], description="Token id that halts generation")
    stop: list[list[int]] | None = Field(None, examples=[None],
                                         description="Stop sequences: up to 16 lists of up to 8 token ids; generation "
                                                     "ends with the first one completed by the generated tokens, "
                                                     "which is kept; null or []: off")
    logit_bias: dict | None = Field(None, examples=[None],
                                                description="Added to the logits of these token ids before "
                                                            "sampling: {\"id\": bias}, each bias in [-100, 100], "
                                                            "at most 1024 ids; null or {}: off")
    banned_token_ids: list | None = Field(None, examples=[None],
                                               description="Token ids that are never generated; null or []: off")
    allowed_token_ids: list | None = Field(None, examples=[None],
                                                description="Generate only these token ids (at least one); "
                                                            "null: no restriction")
    min_tokens: StrictInt | None = Field(None, examples=[None],
                                   description="Generate at least this many tokens before stop_token or a one-token "
                                               "stop sequence may come out; at most max_new_tokens; null or 0: off")
    weight_quant: str | None = Field(None, examples=[None],
                                     description="Decode weight format: \"int8\" (weight-only int8 for batch 1-4 "
                                                 "decode steps), \"\" (bf16), null: PENROZ_DECODE_WEIGHTS")
    speculate: StrictInt | None = Field(None, examples=[None],
                                  description="Prompt-lookup speculative decoding: verify this many draft tokens "
                                              "(1 to 3) per decode step; greedy, one sequence, no stream, prompt + "
                                              "max_new_tokens + speculate <= block_size; the tokens are the plain "
                                              "call's, and \"speculation\" reports steps, drafted and accepted; "
                                              "null or 0: off")
    stream: bool = Field(False, examples=[False], description="Stream tokens as text/plain lines")
    batch: bool = Field(False, examples=[False],
                        description="Return every row: {\"sequences\": [[...], ...]}, each row's prompt plus its "
                                    "tokens; the prompts may differ in length (max length + max_new_tokens <= "
                                    "block_size then); not together with stream")


class DecodeTokensRequest(TokenizerRequest):
    tokens: list[int] = Field(..., examples=[[0]])


class ImportModelRequest(BaseModel):
    hf_repo_id: str = Field(..., examples=["openai-community/gpt2", "google/gemma-3-1b"])
    model_id: str = Field(..., examples=["gpt2-imported"])
    revision: str | None = Field(None, examples=[None])
    device: str = Field("cpu", examples=["cpu", "cuda"])


class ModelIdQuery(Query):
    description = "The unique identifier for the model"


class DatasetIdQuery(Query):
    description = "The unique identifier for the dataset"


# ------------------------------------------------------------------------------ middleware / errors
@app.middleware("http")
async def gzip_decompression_middleware(request: Request, call_next):
    if request.headers.get("Content-Encoding", "").lower() == "gzip":
        body = gzip.decompress(await request.body())
        request._body = body

        async def receive():  # pragma: no cover - exercised through Starlette
            return {"type": "http.request", "body": body, "more_body": False}
        request._receive = receive
    return await call_next(request)


# the process default of /generate's weight_quant is checked once, here: a mistyped
# PENROZ_DECODE_WEIGHTS stops the server at start-up instead of failing every request with a 400
wq_ops.resolve(None)


@app.exception_handler(Exception)
async def generic_exception_handler(_: Request, e: Exception):
    log.error(f"An error occurred: {e}")
    return JSONResponse(status_code=500, content={"detail": "Please refer to server logs"})


@app.exception_handler(KeyError)
async def key_error_handler(_: Request, e: KeyError):
    raise HTTPException(status_code=404, detail=f"Not found error occurred: {e}")


@app.exception_handler(ValueError)
async def value_error_handler(_: Request, e: ValueError):
    raise HTTPException(status_code=400, detail=f"Value error occurred: {e}")


def _json_safe(v):
    """Non-finite floats as text: a 422 echoes the offending input, and NaN / Infinity (which the
    schema refuses, e.g. for the logit penalties) are not JSON."""
    if isinstance(v, float) and not math.isfinite(v):
        return str(v)
    if isinstance(v, dict):
        return {k: _json_safe(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_json_safe(x) for x in v]
    return v


@app.exception_handler(RequestValidationError)
async def validation_error_handler(_: Request, e: RequestValidationError):
    return JSONResponse(status_code=422, content={"detail": jsonable_encoder(_json_safe(e.errors()))})


# ------------------------------------------------------------------------------ serving cache
def serve_device() -> str:
    dev = os.environ.get("PENROZ_SERVE_DEVICE")
    if dev:
        return dev
    try:
        import torch
        return "cuda" if torch.cuda.is_available() else "cpu"
    except Exception:  # pragma: no cover
        return "cpu"


_cache_lock = threading.Lock()
_model_cache: dict[str, tuple[float, NeuralNetworkModel]] = {}


def serving_lock(model: NeuralNetworkModel) -> threading.Lock:
    """The lock every request holds while it runs on ``model``.

    A cached serving model is ONE module tree shared by all requests; generation attaches its
    KV cache / graph decoder to that tree and moves position offsets, so two requests must never
    run on it at once (the reference rebuilt a private model per request, ``main.py:401-434``).
    A plain ``Lock`` (not ``RLock``): a streaming response acquires it on the threadpool thread
    of its first chunk and may release it on another."""
    lk = model.__dict__.get("_serve_lock")
    if lk is None:
        with _cache_lock:
            lk = model.__dict__.setdefault("_serve_lock", threading.Lock())
    return lk


def _lock_timeout_s() -> float:
    return float(os.environ.get("PENROZ_SERVE_LOCK_TIMEOUT", "120"))


class _Held:
    """``with _Held(model):`` — the model's serving lock, waited for at most
    ``PENROZ_SERVE_LOCK_TIMEOUT`` seconds (then 503: busy), never indefinitely."""

    def __init__(self, model):
        self.lock = serving_lock(model)

    def __enter__(self):
        if not self.lock.acquire(timeout=_lock_timeout_s()):
            raise HTTPException(status_code=503, detail="Model is busy serving another request; retry later.")
        return self

    def __exit__(self, *exc):
        self.lock.release()


def _logprob_line(item) -> str:
    """A streamed (token, logprob, [[id, logprob], ...]) as ``token<TAB>logprob`` and one
    ``<TAB>id:logprob`` per top entry; floats by ``repr`` (they read back exactly)."""
    token, lp, top = item
    return "\t".join([str(token), repr(lp)] + [f"{i}:{v!r}" for i, v in top])


class _LockedStream:
    """A token stream that owns the model's serving lock from before the response starts until
    the stream is finished OR abandoned. The response's background task (run by Starlette after
    the body, also when the client disconnected mid-stream) closes the generator — retrying
    while a threadpool thread is still inside it producing a token — so its ``finally`` releases
    the lock at once instead of whenever the abandoned generator is garbage-collected."""

    def __init__(self, model, tokens, line=str):
        self.line = line  # an item of ``tokens`` as the text of its line
        self.lock = serving_lock(model)
        if not self.lock.acquire(timeout=_lock_timeout_s()):
            raise HTTPException(status_code=503, detail="Model is busy serving another request; retry later.")
        self._released = False
        self._guard = threading.Lock()
        self.gen = self._run(tokens)

    def _release(self):
        with self._guard:
            if not self._released:
                self._released = True
                self.lock.release()

    def _run(self, tokens):
        try:
            for token in tokens:
                yield f"{self.line(token)}\n"
        finally:
            self._release()

    def close(self):
        import time
        deadline = time.monotonic() + _lock_timeout_s()
        while True:
            try:
                self.gen.close()  # suspended at a yield (or finished): runs the finally now
                break
            except ValueError:  # "generator already executing" on a threadpool thread
                if time.monotonic() > deadline:
                    return
                time.sleep(0.005)
        self._release()  # never started: the finally never ran


def _checkpoint_mtime(model_id: str) -> float | None:
    p = os.path.join(NeuralNetworkModel.SHM_PATH, NeuralNetworkModel.get_model_path(model_id))
    if not os.path.exists(p):
        p = NeuralNetworkModel.get_model_path(model_id)
    return os.path.getmtime(p) if os.path.exists(p) else None


def load_for_serving(model_id: str) -> NeuralNetworkModel:
    """Deserialize (or reuse) a model and place it on the serving device."""
    if os.environ.get("PENROZ_SERVE_CACHE", "1") != "1":
        model = NeuralNetworkModel.deserialize(model_id)
        dev = serve_device()
        return model.to(dev) if dev != "cpu" and hasattr(model, "to") else model
    mtime = _checkpoint_mtime(model_id)
    with _cache_lock:
        hit = _model_cache.get(model_id)
        if hit is not None and mtime is not None and hit[0] == mtime:
            return hit[1]
    model = NeuralNetworkModel.deserialize(model_id)
    dev = serve_device()
    if dev != "cpu":
        model.to(dev)
    with _cache_lock:
        if mtime is not None:
            while len(_model_cache) >= int(os.environ.get("PENROZ_SERVE_CACHE_SIZE", "2")):
                _model_cache.pop(next(iter(_model_cache)))
            _model_cache[model_id] = (mtime, model)
    return model


def _evict(model_id: str):
    with _cache_lock:
        _model_cache.pop(model_id, None)


# ------------------------------------------------------------------------------ routes
@app.get("/", include_in_schema=False)
def redirect_to_dashboard():
    return RedirectResponse(url="/dashboard")


@app.get("/dashboard", response_class=HTMLResponse, include_in_schema=False)
async def dashboard():
    with open(os.path.join(HERE, "templates", "dashboard.html")) as f:
        return HTMLResponse(f.read())


@app.post("/model/")
def create_model(body: CreateModelRequest = Body(...)):
    model_id = body.model_id
    log.info(f"Requesting creation of model {model_id}")
    model = NeuralNetworkModel(model_id, Mapper(body.layers, body.optimizer))
    model.serialize()
    _evict(model_id)
    return {"message": f"Model {model_id} created and saved successfully"}


@app.post("/import/")
async def import_from_huggingface(body: ImportModelRequest = Body(...)):
    model_id = body.model_id
    lock = model_locks.setdefault(model_id, Lock())
    if lock.locked():
        raise HTTPException(status_code=409, detail=f"Operation already in progress for model {model_id}.")
    async with lock:
        await run_in_threadpool(NeuralNetworkModel.from_huggingface, model_id, body.hf_repo_id, body.revision,
                                body.device)
    _evict(model_id)
    return {"model_id": model_id, "status": "imported",
            "message": f"Model imported from HuggingFace ({body.hf_repo_id}) and ready for use"}


@app.get("/dataset/")
def list_dataset(dataset_id: str = DatasetIdQuery(...)):
    return {"files": Loader(dataset_id).list()}


@app.post("/dataset/")
async def download_dataset(body: DownloadDatasetRequest = Body(...)):
    dataset_id = body.dataset_id
    lock = dataset_locks.setdefault(dataset_id, Lock())
    if lock.locked():
        raise HTTPException(status_code=409, detail=f"Downloading dataset {dataset_id} already in progress.")
    downloader = Downloader(dataset_id, body.shard_size, body.encoding)

    async def download():
        async with lock:
            await run_in_threadpool(downloader.download, body.path, body.name, body.split)

    create_task(download())
    return JSONResponse(content={"message": f"Downloading Dataset {dataset_id} asynchronously."}, status_code=202)


@app.delete("/dataset/")
def delete_dataset(dataset_id: str = DatasetIdQuery(...)):
    Loader(dataset_id).delete()
    return Response(status_code=204)


@app.post("/tokenize/")
def tokenize_text(body: TokenizeTextRequest = Body(...)):
    return {"encoding": body.encoding, "tokens": Tokenizer(body.encoding).tokenize(body.text)}


@app.post("/output/")
def compute_model_output(body: OutputRequest = Body(...)):
    model = load_for_serving(body.model_id)
    with _Held(model):
        output, cost = model.compute_output(body.input, body.target)
    return {"output": output, "cost": cost}


@app.post("/evaluate/")
def evaluate_model(body: EvaluateRequest = Body(...)):
    model = load_for_serving(body.model_id)
    with _Held(model):
        cost = model.evaluate_model(body.dataset_id, body.target_dataset_id, body.shard, body.epochs,
                                    body.batch_size, body.block_size, body.step_size)
    return {"cost": cost}


@app.post("/generate/")
def model_generate(body: GenerateRequest = Body(...)):
    if body.batch and body.stream:  # a 400 before the model is touched
        raise ValueError("batch returns every row at once: not together with stream")
    # (likewise, streams too: an unknown weight format, a malformed stop set, logit bias, banned or allowed set or
    # min_tokens, stop_token together with stop; ids beyond the vocabulary: once the model is loaded and it is known)
    # (and everything a speculative call does not take: its shape is the request's own)
    early = check_options(NOT_LOADED, body.max_new_tokens, body.temperature, body.top_k, body.stop_token,
                          **{name: getattr(body, name) for name in KEYWORDS},
                          call_shape=call_shape_of(body.input, body.block_size, stream=body.stream))
    stop = early.stop
    model = load_for_serving(body.model_id)
    penalties = dict(repetition_penalty=body.repetition_penalty, presence_penalty=body.presence_penalty,
                     frequency_penalty=body.frequency_penalty)
    for name in ("logit_bias", "banned_token_ids", "allowed_token_ids", "min_tokens"):
        if getattr(body, name):  # (a keyword of its own only when the request sets it; {}, [] and 0 are off)
            penalties[name] = getattr(body, name)
    if body.logprobs is not None:  # (a keyword of its own only when asked for: without it the calls are as before)
        penalties["logprobs"] = body.logprobs
    if stop is not None:  # (likewise)
        penalties["stop"] = stop
    if early.speculate:  # (likewise)
        penalties["speculate"] = early.speculate
    if body.batch:
        # every row of the batch, ragged or not (ops/ragged.py): generate_batch's result, row for row
        with _Held(model):
            res = model.generate_batch(body.input, body.block_size, body.max_new_tokens, body.temperature,
                                       body.top_k, body.stop_token, top_p=body.top_p, min_p=body.min_p,
                                       weight_quant=body.weight_quant, **penalties)
            speculation = model.last_speculation
        if early.speculate:
            return {"sequences": res, "speculation": speculation}
        if body.logprobs is None and stop is None:
            return {"sequences": res}
        sequences, infos = res
        out = {"sequences": sequences}
        if stop is not None:
            out["finish_reason"] = [info.pop("finish_reason") for info in infos]
            out["stop_sequence"] = [info.pop("stop_sequence") for info in infos]
        if body.logprobs is not None:
            out["logprobs"] = infos
        return out
    if body.stream:
        # the lock is held for the stream's whole lifetime (the KV cache stays attached between
        # chunks) and released by the background task even when the client goes away mid-stream
        from starlette.background import BackgroundTask
        st = _LockedStream(model, model.generate_tokens_stream(body.input, body.block_size, body.max_new_tokens,
                                                              body.temperature, body.top_k, body.stop_token,
                                                              top_p=body.top_p, min_p=body.min_p,
                                                              weight_quant=body.weight_quant, **penalties),
                           line=str if body.logprobs is None else _logprob_line)
        return StreamingResponse(st.gen, media_type="text/plain", background=BackgroundTask(st.close))
    with _Held(model):
        tokens = model.generate_tokens(body.input, body.block_size, body.max_new_tokens, body.temperature,
                                       body.top_k, body.stop_token, top_p=body.top_p, min_p=body.min_p,
                                       weight_quant=body.weight_quant, **penalties)
        speculation = model.last_speculation
    if early.speculate:
        return {"tokens": tokens, "speculation": speculation}
    if body.logprobs is None and stop is None:
        return {"tokens": tokens}
    tokens, info = tokens
    out = {"tokens": tokens}
    if stop is not None:
        out["finish_reason"], out["stop_sequence"] = info.pop("finish_reason"), info.pop("stop_sequence")
    if body.logprobs is not None:
        out["logprobs"] = info
    return out


@app.post("/decode/")
def decode_tokens(body: DecodeTokensRequest = Body(...)):
    return {"encoding": body.encoding, "text": Tokenizer(body.encoding).decode(body.tokens)}


def _mark_failed(model_id: str, rank: int, code: int):
    try:
        NeuralNetworkModel.mark_status(model_id, "Error", f"Training worker rank {rank} exited with code {code}")
    except Exception as e:  # pragma: no cover - best effort
        log.error(f"could not mark model {model_id} as failed: {e}")


def run_training_job(model_id: str, device: str, dataset_id: str, shard: int, epochs: int, batch_size: int,
                     block_size: int, step_size: int, max_grad_norm: float | None = None) -> int:
    """Blocking: launch the distributed workers and return the launcher's exit code."""
    args = (model_id, device, dataset_id, shard, epochs, batch_size, block_size, step_size)
    if max_grad_norm is not None:  # (absent: the workers get exactly the arguments they always got)
        args += (max_grad_norm,)
    code = launcher.launch_single_node_ddp(
        model_id, device, NeuralNetworkModel.train_model_on_device, *args,
        on_failure=lambda r, c: _mark_failed(model_id, r, c))
    _evict(model_id)
    return code


@app.put("/train/")
async def train_model(body: TrainingRequest = Body(...)):
    model_id = body.model_id
    try:  # before any worker is launched
        max_grad_norm = grad_clip_ops.check_max_grad_norm(body.max_grad_norm)
    except ValueError as e:
        raise HTTPException(status_code=400, detail=f"Value error occurred: {e}")
    lock = model_locks.setdefault(model_id, Lock())
    if lock.locked():
        raise HTTPException(status_code=409, detail=f"Training already in progress for model {model_id}.")

    async def _launch():
        async with lock:
            code = await run_in_threadpool(run_training_job, model_id, body.device, body.dataset_id, body.shard,
                                           body.epochs, body.batch_size, body.block_size, body.step_size,
                                           max_grad_norm)
            log.info(f"Distributed training for model {model_id} finished with exit code {code}")

    create_task(_launch())
    return JSONResponse(content={"message": f"Training for model {model_id} started asynchronously."}, status_code=202)


@app.get("/progress/")
def model_progress(model_id: str = ModelIdQuery(...)):
    doc = NeuralNetworkModel.read_progress(model_id)
    return {"progress": doc["progress"], "average_cost": doc["average_cost"],
            "average_cost_history": doc["average_cost_history"], "status": doc["status"]}


@app.get("/stats/")
def model_stats(model_id: str = ModelIdQuery(...)):
    return NeuralNetworkModel.read_stats(model_id)


@app.delete("/model/")
def delete_model(model_id: str = ModelIdQuery(...)):
    NeuralNetworkModel.delete(model_id)
    _evict(model_id)
    return Response(status_code=204)


def main():  # pragma: no cover - process entry point
    import uvicorn
    from penroz.parallel.dist import load_log_config
    uvicorn.run(app, host=os.environ.get("PENROZ_HOST", "127.0.0.1"), port=int(os.environ.get("PENROZ_PORT", "8000")),
                log_config=load_log_config())


if __name__ == "__main__":  # pragma: no cover
    main()

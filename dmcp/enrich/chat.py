"""The chat turn of a checkpoint: its Jinja chat template, rendered once.

The reference sends each class to a chat model as one user turn
(``ClaudeApiClient.java:306-313``).  An instruct checkpoint only behaves as
trained behind its own turn markers, so the local engine renders the
enrichment prompt through the checkpoint's chat template: one user message,
no system message, the generation prompt appended.

The template is rendered ONCE per engine with a sentinel as the message
content and split on it into :attr:`ChatTemplate.head_text` (everything
before the content: BOS text, a default system block, the user header) and
:attr:`ChatTemplate.tail_text` (end of turn + the assistant header, for
Qwen3 the empty think block).  A prompt is then
``head + content + tail`` with the content tokenised separately -- special
tokens NOT recognised in it, it is untrusted source text
(:meth:`dmcp.enrich.tokenizer.HFTokenizer.encode_plain`).

Where the template comes from, in this order: ``chat_template`` of the
directory's ``tokenizer_config.json`` (a string, or a list of
``{name, template}`` entries of which ``default`` is taken), a
``chat_template.jinja`` file, otherwise none.  A template that does not
compile, does not render a lone user turn, or does not emit the content
exactly once is refused (:class:`dmcp.models.llm.CheckpointUnsupported`,
:func:`template_problem`).  Templates run in Jinja's immutable sandbox.
"""
from __future__ import annotations

import datetime
import json
import os
from dataclasses import dataclass
from typing import Optional, Tuple

ENV_NAME = "LOCAL_LLM_CHAT_TEMPLATE"
# no whitespace at either end (a template's ``| trim`` leaves it alone), no
# character a tokenizer_config.json or a template would plausibly contain
SENTINEL = "⦃dmcp-chat-content-5f1c⦄"


class ChatTemplateError(ValueError):
    """A chat template that cannot be used, with the file it came from."""


@dataclass(frozen=True)
class ChatTemplate:
    source: str        # the file the template was read from
    head_text: str     # rendered text before the user content
    tail_text: str     # rendered text after it (generation prompt included)
    bos_token: str
    eos_token: str


def _token_text(v) -> str:
    """``bos_token`` / ``eos_token`` of a tokenizer_config.json: a plain
    string or an ``{"content": ...}`` object (absent: empty)."""
    if isinstance(v, dict):
        v = v.get("content")
    return v if isinstance(v, str) else ""


def _tokenizer_config(directory: str) -> Tuple[dict, str]:
    path = os.path.join(directory, "tokenizer_config.json")
    if not os.path.isfile(path):
        return {}, path
    try:
        with open(path, encoding="utf-8") as f:
            tc = json.load(f)
    except (OSError, ValueError) as e:
        raise ChatTemplateError(f"{path} cannot be read ({e})") from e
    return (tc if isinstance(tc, dict) else {}), path


def find_template(directory: str) -> Optional[Tuple[str, str]]:
    """(template text, file it came from) of a checkpoint directory, or None."""
    tc, path = _tokenizer_config(directory)
    t = tc.get("chat_template")
    if isinstance(t, list):  # named templates: the default one
        t = next((e.get("template") for e in t if isinstance(e, dict) and e.get("name") == "default"), None)
    if isinstance(t, str) and t:
        return t, path
    path = os.path.join(directory, "chat_template.jinja")
    if os.path.isfile(path):
        with open(path, encoding="utf-8") as f:
            return f.read(), path
    return None


def _environment(now: datetime.datetime):
    from jinja2.sandbox import ImmutableSandboxedEnvironment

    def raise_exception(msg):
        raise ChatTemplateError(str(msg))

    def tojson(x, ensure_ascii=False, indent=None, separators=None, sort_keys=False):
        # plain JSON: Jinja's own filter escapes <, >, & and ' for HTML
        return json.dumps(x, ensure_ascii=ensure_ascii, indent=indent, separators=separators, sort_keys=sort_keys)

    env = ImmutableSandboxedEnvironment(trim_blocks=True, lstrip_blocks=True,
                                        extensions=["jinja2.ext.loopcontrols"])
    env.filters["tojson"] = tojson
    env.globals["raise_exception"] = raise_exception
    env.globals["strftime_now"] = now.strftime  # one timestamp per engine: a run's prompts are constant
    return env


def render_split(template: str, source: str, bos_token: str = "", eos_token: str = "",
                 now: Optional[datetime.datetime] = None) -> ChatTemplate:
    """Renders ``template`` for one user turn whose content is the sentinel
    and splits the result on it.  :class:`ChatTemplateError` naming
    ``source`` when it does not compile, does not render, or emits the
    content other than exactly once."""
    import jinja2
    env = _environment(now or datetime.datetime.now())
    try:
        text = env.from_string(template).render(
            messages=[{"role": "user", "content": SENTINEL}], add_generation_prompt=True,
            bos_token=bos_token, eos_token=eos_token, tools=None,
            # the grammar forces the JSON skeleton from the reply's first token
            enable_thinking=False)
    except jinja2.TemplateSyntaxError as e:
        raise ChatTemplateError(f"chat template of {source} does not compile "
                                f"(line {e.lineno}: {e.message})") from e
    except ChatTemplateError as e:
        raise ChatTemplateError(f"chat template of {source} refuses a lone user turn ({e})") from e
    except Exception as e:  # noqa: BLE001 -- sandbox violations, undefined names, type errors: all refused
        raise ChatTemplateError(f"chat template of {source} does not render "
                                f"({type(e).__name__}: {e})") from e
    n = text.count(SENTINEL)
    if n != 1:
        raise ChatTemplateError(f"chat template of {source} emits the user message's content {n} times, "
                                f"expected exactly once")
    head, tail = text.split(SENTINEL)
    return ChatTemplate(source, head, tail, bos_token, eos_token)


def load_chat_template(directory: str, override: Optional[str] = None,
                       now: Optional[datetime.datetime] = None) -> Optional[ChatTemplate]:
    """The rendered chat turn of a checkpoint directory -- with the template
    of the file ``override`` instead of the directory's own when given; the
    BOS / EOS texts are the directory's either way.  None: no template."""
    tc, _ = _tokenizer_config(directory)
    if override:
        with open(override, encoding="utf-8") as f:
            found = (f.read(), override)
    else:
        found = find_template(directory)
    if found is None:
        return None
    return render_split(found[0], found[1], _token_text(tc.get("bos_token")), _token_text(tc.get("eos_token")), now)


def knob(value) -> str:
    """``LOCAL_LLM_CHAT_TEMPLATE`` normalised: ``auto``, ``off`` or a path."""
    v = str(value if value is not None else "auto").strip()
    return v.lower() if v.lower() in ("auto", "off", "") else v


def template_problem(directory: str, chat_template="auto") -> Optional[str]:
    """Why the chat template the knob selects for ``directory`` cannot be
    used, or None (``off``, no template, or a usable one).  A template file
    that does not exist is not a property of the checkpoint: the engine
    raises for it (:func:`resolve`)."""
    mode = knob(chat_template)
    if mode == "off":
        return None
    override = mode if mode not in ("auto", "") else None
    if override and not os.path.isfile(override):
        return None
    try:
        load_chat_template(directory, override)
    except ChatTemplateError as e:
        return str(e)
    return None


def resolve(tokenizer, chat_template="auto",
            now: Optional[datetime.datetime] = None) -> Tuple[str, Optional[ChatTemplate]]:
    """(mode, template) an engine runs with: ``("raw", None)`` or
    ``("template:<file>", ChatTemplate)``.  ``tokenizer``: the engine's; only
    one loaded from a checkpoint directory (``checkpoint_dir``) can carry a
    template.  ValueError naming the variable for a template file that does
    not exist or is given to a byte / asset tokenizer."""
    mode = knob(chat_template)
    directory = getattr(tokenizer, "checkpoint_dir", None)
    if mode == "off":
        return "raw", None
    if mode in ("auto", ""):
        if not directory:
            return "raw", None
        chat = load_chat_template(directory, None, now)
    else:
        if not os.path.isfile(mode):
            raise ValueError(f"{ENV_NAME}={mode!r}: no such template file (auto, off, or a path to a Jinja file)")
        if not directory or not hasattr(tokenizer, "encode_plain"):
            raise ValueError(f"{ENV_NAME}={mode!r}: a template file needs a checkpoint's own tokenizer "
                             f"(LOCAL_LLM_MODEL_PATH); the byte-level and preset vocabularies have no turn markers")
        chat = load_chat_template(directory, mode, now)
    return ("raw", None) if chat is None else (f"template:{chat.source}", chat)

"""The executor's summarize intent on a fake page and a fake brain: with the knob off the step data is
the reference's note, byte for byte, and nothing is read or posted; with VWA_SUMMARIZE the page's
title, url and visible text (capped at VWA_SUMMARY_PAGE_CHARS) go to the brain's /summarize and the
step carries {summary, chars, truncated, source_chars}; a brain error or a 501 fails the step with
the error's text and ``retries`` re-posts."""
import asyncio
import json

from aiohttp import web
from aiohttp.test_utils import TestServer

from fakes import FakePage
from voice_enabled_browser_automation_amd.executor import actions
from voice_enabled_browser_automation_amd.executor.actions import run_intents

NOTE = {"note": "summarize should be handled by the brain"}
TEXT = "Wireless earbuds are on sale this week.\nFree shipping over $35."


class TextPage(FakePage):
    def __init__(self, text=TEXT, title="Shop", url="https://shop.example/earbuds"):
        super().__init__()
        self.page = {"title": title, "url": url, "text": text}

    async def evaluate(self, script, arg=None):
        if "innerText" in script and "location.href" in script:
            self.calls.append(("page_text",))
            return dict(self.page)
        return await super().evaluate(script, arg)


def run(tmp_path, page, intents, replies, monkeypatch, url_env="VWA_SUMMARIZE_URL"):
    """run_intents against a fake brain that answers ``replies`` (status, body) in turn.  Returns
    (steps, the bodies the brain got)."""
    got = []

    async def summarize(req):
        got.append(await req.json())
        status, body = replies[min(len(got), len(replies)) - 1]
        return web.json_response(body, status=status) if not isinstance(body, str) else web.Response(text=body, status=status)

    real_sleep = asyncio.sleep

    async def no_sleep(_s, *a, **k):
        return await real_sleep(0)

    async def go():
        app = web.Application()
        app.router.add_post("/summarize", summarize)
        async with TestServer(app) as srv:
            if url_env == "BRAIN_URL":  # derived: /parse replaced by /summarize
                monkeypatch.setenv("BRAIN_URL", str(srv.make_url("/parse")))
            else:
                monkeypatch.setenv(url_env, str(srv.make_url("/summarize")))
            monkeypatch.setattr(actions.asyncio, "sleep", no_sleep)  # (the pause between attempts)
            return await run_intents(page, str(tmp_path), intents, upload_dir=str(tmp_path / "up"))

    return asyncio.run(go()), got


def intent(**kw):
    return {"type": "summarize", "args": {}, "priority": 0, "requires_confirmation": False, **kw}


OK = (200, {"summary": "Earbuds are on sale, with free shipping.", "chars": 40, "truncated": False, "page_tokens": 17})


def test_with_the_knob_off_the_step_is_the_reference_note(tmp_path, monkeypatch):
    monkeypatch.delenv("VWA_SUMMARIZE", raising=False)
    page = TextPage()
    steps, got = run(tmp_path, page, [intent()], [OK], monkeypatch)
    assert got == [] and page.calls == []
    assert json.dumps(steps[0]["data"]) == '{"note": "summarize should be handled by the brain"}'
    assert steps[0]["data"] == NOTE and steps[0]["ok"] is True and steps[0]["attempts"] == 1
    monkeypatch.setenv("VWA_SUMMARIZE", "0")
    steps, got = run(tmp_path, page, [intent()], [OK], monkeypatch)
    assert got == [] and steps[0]["data"] == NOTE


def test_with_the_knob_on_the_page_goes_to_the_brain_and_the_summary_comes_back(tmp_path, monkeypatch):
    monkeypatch.setenv("VWA_SUMMARIZE", "1")
    page = TextPage()
    steps, got = run(tmp_path, page, [intent()], [OK], monkeypatch)
    assert got == [{"text": TEXT, "title": "Shop", "url": "https://shop.example/earbuds"}]
    assert steps[0]["ok"] is True and steps[0]["data"] == {
        "summary": OK[1]["summary"], "chars": 40, "truncated": False, "source_chars": len(TEXT)}
    assert page.calls == [("page_text",)]
    # the URL derived from BRAIN_URL; args.max_chars is passed on; truncated is reported
    monkeypatch.delenv("VWA_SUMMARIZE_URL", raising=False)
    steps, got = run(tmp_path, TextPage(), [intent(args={"max_chars": 120})],
                     [(200, dict(OK[1], truncated=True))], monkeypatch, url_env="BRAIN_URL")
    assert got[0]["max_chars"] == 120 and steps[0]["data"]["truncated"] is True
    assert actions.summarize_url().endswith("/summarize")
    monkeypatch.setenv("BRAIN_URL", "http://127.0.0.1:8090/parse")
    assert actions.summarize_url() == "http://127.0.0.1:8090/summarize"
    monkeypatch.setenv("BRAIN_URL", "http://brain:8090")
    assert actions.summarize_url() == "http://brain:8090/summarize"


def test_the_page_cap_is_applied(tmp_path, monkeypatch):
    monkeypatch.setenv("VWA_SUMMARIZE", "1")
    monkeypatch.setenv("VWA_SUMMARY_PAGE_CHARS", "100")
    text = "0123456789" * 50
    steps, got = run(tmp_path, TextPage(text="  " + text + "\n"), [intent()], [OK], monkeypatch)
    assert got[0]["text"] == text[:100]
    assert steps[0]["data"]["source_chars"] == 500 and steps[0]["ok"] is True


def test_a_brain_error_fails_the_step_and_retries_reposts(tmp_path, monkeypatch):
    monkeypatch.setenv("VWA_SUMMARIZE", "1")
    err = (500, {"error": "llm_error", "detail": "kv cache exhausted"})
    steps, got = run(tmp_path, TextPage(), [intent()], [err], monkeypatch)
    assert len(got) == 1 and steps[0]["ok"] is False and "data" not in steps[0]
    assert "500" in steps[0]["error"] and "kv cache exhausted" in steps[0]["error"]
    # retries: the second post succeeds
    steps, got = run(tmp_path, TextPage(), [intent(retries=2)], [err, OK], monkeypatch)
    assert len(got) == 2 and steps[0]["ok"] is True and steps[0]["attempts"] == 2 and "error" not in steps[0]
    assert steps[0]["data"]["summary"] == OK[1]["summary"]
    # an engine without summaries, a reply that is not JSON, a reply without a summary
    steps, got = run(tmp_path, TextPage(), [intent(retries=1)], [(501, {"error": "summarize_unsupported"})], monkeypatch)
    assert len(got) == 2 and steps[0]["ok"] is False and "501" in steps[0]["error"] \
        and "summarize_unsupported" in steps[0]["error"]
    for bad in ((200, "not json"), (200, {"chars": 3}), (200, {"summary": 7})):
        steps, _ = run(tmp_path, TextPage(), [intent()], [bad], monkeypatch)
        assert steps[0]["ok"] is False and "summarize" in steps[0]["error"]


def test_a_page_without_visible_text_fails_the_step_before_any_post(tmp_path, monkeypatch):
    monkeypatch.setenv("VWA_SUMMARIZE", "1")
    steps, got = run(tmp_path, TextPage(text="  \n "), [intent()], [OK], monkeypatch)
    assert got == [] and steps[0]["ok"] is False and "no visible text" in steps[0]["error"]
    # the other intents around it still run
    steps, got = run(tmp_path, TextPage(), [{"type": "back", "args": {}}, intent(), {"type": "back", "args": {}}], [OK],
                     monkeypatch)
    assert [s["ok"] for s in steps] == [True, True, True] and len(got) == 1
